"""Survey-level entry (reduced to what feeds the path): the reference's user inputs -- an options file
and an FDEM or TDEM data CSV -- to the posteriors of every sounding, on the GPUs of one node.

Mirrors what the reference's harness does around ``Inference1D`` without its control plane:
  ``read_options``      inversion/user_parameters.py:31-99 (same keys, same defaults, same required keys)
  ``FdemData.read_csv`` classes/data/dataset/FdemData.py:620-682 + Data.py:505-528 + pointcloud/Point.py:355-382
                        (column recognition by header name), one row per sounding
  ``TdemData.read_csv`` classes/data/dataset/TdemData.py (columns S<system><component>_time_<t>, txrx_d{x,y,z})
  ``infer``             inversion/Inference3D.py:518-635: soundings are independent; a rank owns one GPU and a
                        contiguous block of soundings (base/MPI.py:172-201) and runs all of its chains in lockstep
                        (``DeviceChains`` under the reference's burn-in / stop schedule); results are gathered on rank 0.
The reference's HDF5 output (row f-4) is not reproduced: results are numpy arrays (``SurveyResult.save`` -> .npz).
"""
import ast
import os

import numpy as np

from .datapoint import FdemDataPoint
from .system import FdemSystem

REQUIRED_KEYS = ("data_type", "data_filename", "system_filename", "n_markov_chains", "interactive_plot", "update_plot_every",
                 "save_png", "save_hdf5", "solve_parameter", "solve_gradient", "maximum_number_of_layers", "minimum_depth",
                 "maximum_depth", "probability_of_birth", "probability_of_death", "probability_of_perturb",
                 "probability_of_no_change")
_DATA_TYPES = ("FdemData", "TdemData", "TempestData", "FdemDataPoint", "TdemDataPoint", "TempestDataPoint")


def _value(node):
    """Literals, arithmetic on literals, lists / tuples, and the data-type names (kept as strings).  The reference
    exec()s the file (user_parameters.py:83-88); the files it ships need no more than this."""
    if isinstance(node, ast.Name):
        if node.id in _DATA_TYPES:
            return node.id
        if node.id in ("inf", "nan"):
            return float(node.id)
        raise ValueError("unknown name {!r} in options file".format(node.id))
    if isinstance(node, (ast.List, ast.Tuple)):
        return [_value(e) for e in node.elts]
    if (isinstance(node, ast.Subscript) and isinstance(node.value, ast.Attribute) and node.value.attr == "r_"
            and isinstance(node.value.value, ast.Name) and node.value.value.id in ("np", "numpy")):
        # np.r_[a, b, ...] of the reference's tempest_options (per-channel additive errors): a flat list of numbers
        sl = node.slice
        parts = [_value(e) for e in sl.elts] if isinstance(sl, ast.Tuple) else [_value(sl)]
        return [float(x) for q in parts for x in (q if isinstance(q, list) else [q])]
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
        v = _value(node.operand)
        return -v if isinstance(node.op, ast.USub) else v
    if isinstance(node, ast.BinOp):
        a, b = _value(node.left), _value(node.right)
        ops = {ast.Add: lambda: a + b, ast.Sub: lambda: a - b, ast.Mult: lambda: a * b, ast.Div: lambda: a / b,
               ast.Pow: lambda: a ** b}
        if type(node.op) not in ops:
            raise ValueError("unsupported operator in options file")
        return ops[type(node.op)]()
    return ast.literal_eval(node)


def read_options(filename, **overrides):
    """dict of the options file's assignments with the reference's defaults filled in and the file names joined to
    ``data_directory`` (relative directories are taken relative to the options file)."""
    with open(filename) as f:
        tree = ast.parse(f.read(), filename=filename)
    o = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            o[node.targets[0].id] = _value(node.value)
    o.update({k: v for k, v in overrides.items() if v is not None})
    missing = [k for k in REQUIRED_KEYS if k not in o]
    if missing:
        raise ValueError("Missing {} from the user parameter file".format(missing))
    for key, default in (("gradient_standard_deviation", 1.5), ("multiplier", 1.0), ("factor", 10.0), ("covariance_scaling", 1.0)):
        if o.get(key) is None:
            o[key] = default
    o["stochastic_newton"] = not o.get("ignore_likelihood", False)
    base = o.get("data_directory", "")
    if not os.path.isabs(base):
        base = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(filename)), base))
    join = lambda v: [os.path.join(base, x) for x in v] if isinstance(v, list) else os.path.join(base, v)
    o["data_filename"], o["system_filename"] = join(o["data_filename"]), join(o["system_filename"])
    return o


class FdemData:
    """A set of FDEM soundings (classes/data/dataset/FdemData.py): per-sounding location, altitude and the 2 F data
    channels [in-phase F | quadrature F] in ppm, optional standard deviations."""

    def __init__(self, system, lineNumber, fiducial, x, y, z, elevation, data, std=None):
        self.system = system if isinstance(system, FdemSystem) else FdemSystem.read(system)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.lineNumber, self.fiducial = f64(lineNumber), f64(fiducial)
        self.x, self.y, self.z, self.elevation = f64(x), f64(y), f64(z), f64(elevation)
        self.data = f64(data)
        self.std = None if std is None else f64(std)
        assert self.data.shape == (self.nPoints, 2 * self.system.nFrequencies), ValueError(
            "data must have shape (nPoints, 2 * nFrequencies)")

    @property
    def nPoints(self):
        return self.x.size

    @property
    def nChannels(self):
        return self.data.shape[1]

    @staticmethod
    def _csv_channels(header):
        """Column roles by header name, the reference's rules (case-insensitive)."""
        roles = dict(line=("line", "linenumber", "line_number"), fid=("fid", "fiducial", "id"), x=("e", "x", "easting"),
                     y=("n", "y", "northing"), z=("alt", "altitude", "laser", "bheight", "height"),
                     elev=("dtm", "dem_elev", "dem_np", "topo", "elev", "elevation"))
        loc, inphase, quad, in_err, quad_err = {}, [], [], [], []
        for j, name in enumerate(header):
            c = name.strip().lower()
            role = next((r for r, names in roles.items() if c in names), None)
            if role is not None:
                loc[role] = j
            elif any(label in c for label in ("cpi", "i_", "in_phase")):
                (in_err if "err" in c else inphase).append(j)
            elif any(label in c for label in ("cpq", "q_", "quad")):
                (quad_err if "err" in c else quad).append(j)
        if "line" not in loc or "fid" not in loc:
            raise ValueError("File must contain columns for line and fiducial")
        if not all(r in loc for r in ("x", "y", "z")):
            raise ValueError("File must contain columns for easting, northing, height. May also have an elevation column")
        return loc, inphase + quad, in_err + quad_err

    @classmethod
    def read_csv(cls, data_filename, system_filename):
        system = system_filename if isinstance(system_filename, FdemSystem) else FdemSystem.read(system_filename)
        with open(data_filename) as f:
            first = f.readline()
        sep = "," if "," in first else None
        header = [h for h in (first.strip().split(sep) if sep else first.split())]
        loc, dcols, ecols = cls._csv_channels(header)
        if len(dcols) != 2 * system.nFrequencies:
            raise ValueError("Number of data columns {} in {} does not match 2 * nFrequencies {}".format(
                len(dcols), data_filename, 2 * system.nFrequencies))
        table = np.atleast_2d(np.loadtxt(data_filename, delimiter=sep, skiprows=1))
        col = lambda r: table[:, loc[r]]
        elev = col("elev") if "elev" in loc else np.zeros(table.shape[0])
        std = table[:, ecols] if len(ecols) == len(dcols) else None
        return cls(system, col("line"), col("fid"), col("x"), col("y"), col("z"), elev, table[:, dcols], std)

    def subset(self, rows):
        return FdemData(self.system, self.lineNumber[rows], self.fiducial[rows], self.x[rows], self.y[rows], self.z[rows],
                        self.elevation[rows], self.data[rows], None if self.std is None else self.std[rows])

    def datapoint(self, i):
        """Sounding i as the per-sounding object (FdemData.datapoint, FdemData.py:447-487)."""
        return FdemDataPoint(x=self.x[i], y=self.y[i], z=self.z[i], elevation=self.elevation[i], data=self.data[i],
                             std=None if self.std is None else self.std[i], system=self.system,
                             lineNumber=self.lineNumber[i], fiducial=self.fiducial[i])


class TdemData:
    """A set of time-domain soundings (classes/data/dataset/TdemData.py): location, altitude, transmitter-receiver offset and
    the window data of every system, columns ``S<system><component>_time_<t>`` of the reference's CSV files in file order
    (system 0 component X then Z windows, system 1 ...), which is TdemBatch's channel layout.  ``offset``: one (dx, dy, dz) for
    the set or one per sounding [nPoints, 3] (columns txrx_dx / dy / dz); the Hankel tables depend on it, so ``infer`` builds one
    table set per distinct (horizontal distance, dz) and every chain runs with its own.  ``primary_field`` [nPoints, components]:
    the PX / PY / PZ columns of Tempest files (TempestData.py), kept for the caller, NaN when absent.  ``loop_angles``
    [nPoints, 6]: the file's tx_pitch, tx_roll, tx_yaw, rx_pitch, rx_roll, rx_yaw columns (degrees, the reference's own
    convention; TdemData.py:588-589); ``attitude`` is what Loop_pair.Geometry hands GA-AEM from them (roll, -pitch, -yaw per
    loop, Loop_pair.py:70-77) and what the kernels' geometry mixing takes."""

    MAX_OFFSET_SETS = 4096

    def __init__(self, system, lineNumber, fiducial, x, y, z, elevation, data, offset, primary_field=None, loop_angles=None):
        from .tdem import TdemSystem
        systems = [system] if isinstance(system, (str, TdemSystem)) else list(system)
        self.system = [s if isinstance(s, TdemSystem) else TdemSystem(s) for s in systems]
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.lineNumber, self.fiducial = f64(lineNumber), f64(fiducial)
        self.x, self.y, self.z, self.elevation = f64(x), f64(y), f64(z), f64(elevation)
        self.data = f64(data)
        off = np.asarray(offset, dtype=np.float64)
        self.offsets = np.array(np.broadcast_to(off, (self.x.size, 3)), dtype=np.float64)      # per sounding (own, writable copy)
        self.primary_field = None if primary_field is None else f64(primary_field)
        self.loop_angles = np.zeros((self.x.size, 6)) if loop_angles is None else np.array(np.broadcast_to(f64(loop_angles), (self.x.size, 6)))
        n = sum(s.n_components * s.nwindows for s in self.system)
        assert self.data.shape == (self.nPoints, n), ValueError("data must have shape (nPoints, {})".format(n))

    @property
    def nPoints(self):
        return self.x.size

    @property
    def nChannels(self):
        return self.data.shape[1]

    @property
    def attitude(self):
        """[nPoints, 6] (tx roll, pitch, yaw, rx roll, pitch, yaw) in GA-AEM's convention (Loop_pair.py:70-77)."""
        a = self.loop_angles
        return np.stack([a[:, 1], -a[:, 0], -a[:, 2], a[:, 4], -a[:, 3], -a[:, 5]], axis=1)

    @property
    def offset(self):
        """The one transmitter-receiver offset of the set (raises when the soundings do not share one)."""
        assert np.all(self.offsets == self.offsets[0]), ValueError("the soundings have different transmitter-receiver offsets; use .offsets")
        return tuple(float(v) for v in self.offsets[0])

    def offset_groups(self, rows=None):
        """[(offset triple, row indices)] of the distinct offsets among ``rows`` (default: all), in order of first appearance."""
        rows = np.arange(self.nPoints) if rows is None else np.asarray(rows)
        uniq, first, inverse = np.unique(self.offsets[rows], axis=0, return_index=True, return_inverse=True)
        order = np.argsort(first)
        return [(tuple(float(v) for v in uniq[g]), rows[np.nonzero(inverse.ravel() == g)[0]]) for g in order]

    @classmethod
    def read_csv(cls, data_filename, system_filename):
        with open(data_filename) as f:
            header = [h.strip() for h in f.readline().strip().split(",")]
        low = [h.lower() for h in header]
        find = lambda names: next(j for j, h in enumerate(low) if h in names)
        roles = dict(line=("line", "linenumber", "line_number"), fid=("fid", "fiducial", "id"), x=("e", "x", "easting"),
                     y=("n", "y", "northing"), z=("alt", "altitude", "laser", "bheight", "height"))
        idx = {r: find(names) for r, names in roles.items()}
        elev = next((j for j, h in enumerate(low) if h in ("dtm", "dem_elev", "dem_np", "topo", "elev", "elevation")), None)
        # data columns: the reference's rule (TdemData.py:622-631): a header containing off_time / x_time / y_time / z_time is a
        # window of the secondary field, unless it also contains 'err' (an error column, not read here)
        is_win = lambda h: any(t in h for t in ("off_time", "x_time", "y_time", "z_time"))
        dcols = [j for j, h in enumerate(low) if is_win(h) and "err" not in h]
        if not dcols:
            raise ValueError("{}: no data columns (headers containing off_time, x_time, y_time or z_time); found {}".format(
                data_filename, header))
        table = np.atleast_2d(np.loadtxt(data_filename, delimiter=",", skiprows=1))
        off = np.stack([table[:, low.index(k)] for k in ("txrx_dx", "txrx_dy", "txrx_dz")], axis=1)
        pcols = sorted(j for j, h in enumerate(low) if h in ("px", "py", "pz"))            # TdemData.py:632, primary_channels.sort()
        angles = np.stack([table[:, low.index(k)] if k in low else np.zeros(table.shape[0])
                           for k in ("tx_pitch", "tx_roll", "tx_yaw", "rx_pitch", "rx_roll", "rx_yaw")], axis=1)
        c = lambda r: table[:, idx[r]]
        return cls(system_filename, c("line"), c("fid"), c("x"), c("y"), c("z"),
                   table[:, elev] if elev is not None else np.zeros(table.shape[0]), table[:, dcols], off,
                   primary_field=table[:, pcols] if pcols else None, loop_angles=angles)

    def subset(self, rows):
        return type(self)(self.system, self.lineNumber[rows], self.fiducial[rows], self.x[rows], self.y[rows], self.z[rows],
                          self.elevation[rows], self.data[rows], self.offsets[rows],
                          primary_field=None if self.primary_field is None else self.primary_field[rows], loop_angles=self.loop_angles[rows])


class TempestData(TdemData):
    """Fixed-wing Tempest soundings (classes/data/dataset/TempestData.py): the same file layout with X and Z components, the
    per-sounding transmitter-receiver offsets and the primary-field columns PX / PZ.  The reference's Tempest data point works
    on TOTAL fields -- channel = secondary + the component's primary (Tempest_datapoint.py:106-123) -- with per-channel
    additive errors scaled by a multiplier per component (:161-176): ``total_field`` gives those channels."""

    def total_field(self, rows=None):
        rows = slice(None) if rows is None else rows
        d = self.data[rows]
        if self.primary_field is None:
            return d
        nc = self.primary_field.shape[1]
        return d + np.repeat(self.primary_field[rows], d.shape[1] // nc, axis=1)


class SurveyResult(dict):
    """Per-sounding results, rows in file order: line, fiducial, x, y, z, elevation, status (1 done, 2 failed to burn
    in), burned_in_iteration, iterations, acceptance, misfit, relative_error, additive_error, n_layers, best_* (highest
    posterior model: n_layers, edges, conductivity), layer_count_posterior [S, K + 1], interface_posterior
    [S, n_depth_bins], depth_bin_width, and -- when the hit map is kept -- mean_log10_conductivity [S, n_depth_bins] and
    the 5 / 50 / 95 % conductivity percentiles per depth cell."""

    def save(self, filename):
        from .hdf import save_npz
        save_npz(filename, self, threads=max(1, min(8, _usable_cores())))     # (.npz, deflate level 1, members side by side: hdf.save_npz)

    @classmethod
    def load(cls, filename):
        """A result written by ``save`` / ``save_lines`` (scalars come back as Python scalars)."""
        with np.load(filename, allow_pickle=False) as f:
            return cls({k: (f[k].item() if f[k].ndim == 0 else f[k]) for k in f.files})

    @classmethod
    def load_lines(cls, directory):
        """The per-line files of ``save_lines`` put back together, lines in ascending order (rows keep their order within a line)."""
        names = sorted((n for n in os.listdir(directory) if n.endswith(".npz")), key=lambda n: float(n[:-4]))
        parts = [cls.load(os.path.join(directory, n)) for n in names]
        S = [p["line"].size for p in parts]
        out = cls()
        for k, v in parts[0].items():
            per_row = isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == S[0]
            out[k] = np.concatenate([p[k] for p in parts], axis=0) if per_row else v
        return out

    def save_lines(self, directory):
        """One file per flight line, ``<line number>.npz`` (the reference writes ``<line number>.h5`` there)."""
        from .hdf import save_npz
        S = self["line"].size
        paths = []
        for ln in np.unique(self["line"]):
            m = self["line"] == ln
            part = {k: (v[m] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == S else v) for k, v in self.items()}
            paths.append(os.path.join(directory, "{}.npz".format(ln)))
            save_npz(paths[-1], part)
        return paths


def _hitmap_statistics(hitmap, log_mean_prior, half_width):
    """Mean and percentiles of log10 conductivity per depth cell from the hit map (the reference derives the same from
    its Histogram2D posterior): one kernel over the maps, geobipy_amd.hitmap."""
    from .hitmap import statistics
    return statistics(hitmap, log_mean_prior, half_width)


def _usable_cores():
    """Host cores this process may really use: the scheduler affinity capped by the cgroup CPU quota (a 16-CPU quota on a 256-thread
    host: more writer threads than that only contend)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(round(int(quota) / int(period)))))
    except (OSError, ValueError):
        pass
    return n


def _container_kind(ds):
    return "tempest" if isinstance(ds, TempestData) else ("tdem" if isinstance(ds, TdemData) else "fdem")


def _row_fields(ds, dc, hitmap):
    """The columns of a finished block's device rows for this data set and sampler: hdf.device_row_fields' two lists [(name, width)],
    float64 and int32, and the keyword arguments they were asked with.  The one place that decides them: survey_run's payload packs the
    rows in this order and _LineWriter reads them in it (``hitmap`` False: the hit maps travel apart, as runs)."""
    from . import hdf
    td = _container_kind(ds) != "fdem"
    fkw = dict(hitmap=hitmap, n_rel=dc.n_rel_groups, n_add=dc.n_add_groups, time_domain=td,
               n_primary=(ds.primary_field.shape[1] if getattr(ds, "primary_field", None) is not None else 0) if td else 0,
               height=bool(getattr(dc, "solve_height", False)), angles=tuple((m_[0], m_[5]) for m_ in (getattr(dc, "_moves", None) or ())),
               trace_length=int(getattr(dc, "trace_length", 0) or 0))
    ff, fi = hdf.device_row_fields(dc.N, dc.K, dc.n_depth_bins, dc.n_value_bins, **fkw)
    return ff, fi, fkw


class _LineWriter:
    """Fills one results container per flight line (geobipy_amd.hdf) from chunks of device rows; a line's container is compressed and
    written out by a writer thread, and dropped, as soon as its last sounding has arrived -- what is held is the open lines."""

    def __init__(self, directory, ds, o, dc, hitmap, container=None):
        from concurrent.futures import ThreadPoolExecutor
        from . import hdf
        os.makedirs(directory, exist_ok=True)
        self.hdf, self.directory, self.ds, self.o, self.hitmap = hdf, directory, ds, o, hitmap
        self.container = hdf.container_type(container)        # "hdf5" (<line>.h5) | "npz" (<line>.results.npz + .attrs.json)
        self.K, self.N, self.nd, self.nv = dc.K, dc.N, dc.n_depth_bins, dc.n_value_bins
        kind = self.kind = _container_kind(ds)
        ff, fi, fkw = _row_fields(ds, dc, hitmap)
        n_primary, height, angles = fkw["n_primary"], fkw["height"], fkw["angles"]
        self.trace_every, self.trace_length = int(getattr(dc, "trace_every", 0) or 0), fkw["trace_length"]
        # int32 rows come with dense hit-map columns (wi_dense: rows streamed from other ranks) or without (wi: the hit maps travel as
        # their non-zero entries); hm_tail = the columns after the hit map's
        self.wf, self.wi_dense = sum(w for _, w in ff), sum(w for _, w in fi)
        names_i = [n_ for n_, _ in fi]
        self.hm_tail = sum(w for _, w in fi[names_i.index("hitmap") + 1:]) if hitmap else 0
        self.wi = self.wi_dense - (self.nv * self.nd if hitmap else 0)
        self.line_col = [n_ for n_, _ in ff].index("line_number")
        self.fid_col = [n_ for n_, _ in ff].index("fiducial")
        self.wkw = dict(hitmap=hitmap, kind=kind, n_rel=dc.n_rel_groups, n_add=dc.n_add_groups, n_primary=n_primary,
                        loop_radius=ds.system[0].loopRadius() if fkw["time_domain"] else 0.0,
                        channel_additive=o.get("initial_additive_error") if kind == "tempest" else None, height=height, angles=angles,
                        trace_length=self.trace_length)
        self.lines, self.paths = {}, []
        # finished lines are compressed and written by a few host threads (zlib releases the interpreter lock) while the next rows
        # arrive; at most 2 x workers lines wait for their turn, so the process still holds a bounded number of lines
        self.workers = max(1, min(16, _usable_cores() - 1))
        self.pool, self.pending = ThreadPoolExecutor(max_workers=self.workers), []

    def _close(self, ln):
        root, fid, path, _ = self.lines.pop(ln)
        if isinstance(root, self.hdf.NpzGroup):
            while len(self.pending) >= 2 * self.workers:
                self.pending.pop(0).result()
            self.pending.append(self.pool.submit(root.save, path))   # <line>.h5, or <line>.results.npz (+ <line>.results.attrs.json)
            self.paths.append(path if root.container == "hdf5" else path + ".npz")
        else:
            root.close()
            self.paths.append(path)

    def add(self, f, i, csr=None):
        """Rows of hdf.device_row_fields (numpy [m, wf] float64, [m, wi] int32) of any lines; ``csr`` = (ptr, index, value): the
        rows' hit maps in run-length form (hdf._Dataset.write_run_rows; the int32 rows then carry no hit-map columns)."""
        hdf, ds = self.hdf, self.ds
        if csr is None and self.hitmap:               # dense hit-map columns (rows streamed from other ranks): the same run-length form
            c0 = self.wi_dense - self.hm_tail - self.nv * self.nd
            hm = i[:, c0:c0 + self.nv * self.nd]
            edge = np.ones(hm.shape, dtype=bool)     # run starts: a row's first cell and every change of value
            edge[:, 1:] = hm[:, 1:] != hm[:, :-1]
            r_, j_ = np.nonzero(edge)
            csr = (np.r_[0, np.cumsum(np.bincount(r_, minlength=hm.shape[0]))], j_.astype(np.int32), hm[r_, j_])
            i = np.concatenate([i[:, :c0], i[:, c0 + self.nv * self.nd:]], axis=1)
        for ln in np.unique(f[:, self.line_col]):
            if ln not in self.lines:
                fid = np.sort(ds.fiducial[ds.lineNumber == ln])
                path = hdf.results_path(self.directory, ln, container=self.container)     # <line>.h5, or <line>.results(.npz) for the stand-in
                root = hdf.open_results(path, container=self.container)
                hdf.create_inference1d(root, hdf.LineSpec(ds.system, self.N, self.o, n_value_bins=self.nv, kind=self.kind,
                                                          trace_every=max(1, self.trace_every)), add_axis=fid)
                self.lines[ln] = [root, fid, path, 0]
            root, fid, _, _ = self.lines[ln]
            m = f[:, self.line_col] == ln
            rows_ = np.flatnonzero(m)
            run = rows_[-1] - rows_[0] + 1 == rows_.size       # the line's rows are one run of the chunk (the usual case): views, no copies
            fm, im = (f[rows_[0]:rows_[-1] + 1], i[rows_[0]:rows_[-1] + 1]) if run else (f[m], i[m])
            sub = csr
            if csr is not None and rows_.size != f.shape[0]:       # the line's rows of the chunk's run-length block
                ptr_, ind_, val_ = csr
                if run:
                    a_, b_ = int(ptr_[rows_[0]]), int(ptr_[rows_[-1] + 1])
                    sub = (ptr_[rows_[0]:rows_[-1] + 2] - a_, ind_[a_:b_], val_[a_:b_])
                else:
                    take = np.concatenate([np.arange(ptr_[q_], ptr_[q_ + 1]) for q_ in rows_])
                    sub = (np.r_[0, np.cumsum(np.diff(ptr_)[rows_])], ind_[take], val_[take])
            hdf.write_device_rows(root, np.searchsorted(fid, fm[:, self.fid_col]), fm, im, self.N, self.K, self.nd, self.nv, self.o,
                                  hitmap_csr=sub, **self.wkw)
            self.lines[ln][3] += int(rows_.size)
            if self.lines[ln][3] >= fid.size:
                self._close(ln)

    def add_block(self, block):
        """One finished block of this process: survey_run's payload() -- (rows, float64 rows, int32 rows) on the host with dense hit-map columns,
        taken 64 rows at a time, or (rows, float64 rows, int32 rows, (ptr, index, value)) with the hit maps as their non-zero
        entries, taken whole (the rows of a line are then one slice of each array)."""
        f_b, i_b = block[1], block[2]
        csr = block[3] if len(block) > 3 else None
        f_np, i_np = f_b.numpy(), i_b.numpy()      # (host tensors: views; nothing collective here -- ranks that own whole lines call
        assert f_b.shape[1] == self.wf             #  this as often as they have blocks)
        if csr is not None:
            assert i_b.shape[1] == self.wi
            if f_np.shape[0]:
                self.add(f_np, i_np, csr)
            return
        assert i_b.shape[1] == self.wi_dense
        for a in range(0, f_np.shape[0], 64):
            self.add(f_np[a:a + 64], i_np[a:a + 64])

    def finish(self):
        for ln in list(self.lines):
            self._close(ln)
        for job in self.pending:
            job.result()                           # (re-raises what a writer thread raised)
        self.pool.shutdown()
        return self.paths


def _write_line_containers(directory, ds, o, dc, shipped, hitmap, rank, container=None):
    """Several ranks: rank 0 receives every rank's rows chunk by chunk (ONE exchange: every rank enters it once, whatever number of
    blocks the dynamic schedule gave it) and fills the line containers (_LineWriter).  (One process writes its blocks as they
    finish: infer.)"""
    import torch
    from .distributed import stream_rows_to_root
    w = _LineWriter(directory, ds, o, dc, hitmap, container)
    cat = lambda j, wd, dt: torch.cat([s_[j] for s_ in shipped]) if shipped else torch.zeros((0, wd) if wd else (0,), dtype=dt)
    rows_t, f_t, i_t = cat(0, 0, torch.int64), cat(1, w.wf, torch.float64), cat(2, w.wi_dense, torch.int32)
    assert f_t.shape[1] == w.wf and i_t.shape[1] == w.wi_dense
    if dc.device.type != "cpu" and torch.distributed.is_initialized() and torch.distributed.get_backend() != "gloo":
        rows_t, f_t, i_t = rows_t.to(dc.device), f_t.to(dc.device), i_t.to(dc.device)     # RCCL sends device memory, 64 rows at a time
    for _, (f, i) in stream_rows_to_root(rows_t, [f_t, i_t], chunk_rows=64):
        w.add(f, i)
    return w.finish()


def select_soundings(ds, index=None, fiducial=None, line_number=None):
    """Row indices chosen by the reference's --index / --fiducial / --line switches (Inference3D.infer_serial :458-500:
    one data point by position, or by fiducial on a line); all rows when none is given."""
    if index is not None:
        assert 0 <= index < ds.nPoints, ValueError("index {} outside the {} data points".format(index, ds.nPoints))
        return np.array([index])
    if fiducial is not None:
        assert line_number is not None, ValueError("--fiducial needs --line")
        hit = np.nonzero((ds.fiducial == fiducial) & (ds.lineNumber == line_number))[0]
        assert hit.size > 0, ValueError("fiducial {} not found on line {}".format(fiducial, line_number))
        return hit[:1]
    if line_number is not None:
        hit = np.nonzero(ds.lineNumber == line_number)[0]
        assert hit.size > 0, ValueError("line {} not found".format(line_number))
        return hit
    return np.arange(ds.nPoints)


# the per-sounding summaries a run with replicate chains adds, in the order of the result rows (replicates.Pooled.diagnostics)
REPLICATE_SUMMARIES = ("rhat", "jsd", "n_used", "chain_mean", "rhat_layers", "jsd_layers", "rhat_interfaces", "rhat_max")

BLOCK_PAYLOAD_BUDGET = 8 << 30      # bytes of traces + hit maps one device block may hold by default (infer's ``chunk``)


def infer(options, output=None, seed=None, device=None, hitmap=True, burn_in_min_iterations=5000, check_every=1000,
          exact_jacobian=False, data=None, index=None, fiducial=None, line_number=None, hankel_eps=None, schedule="static",
          chunk=None, results_directory=None, timings=None, traces=1, container=None, units=None, unit_kinds=("arithmetic", "harmonic"),
          first_above=(), first_below=(), replicates=1, data_posteriors=None, ensemble=None, ensemble_diagnostics=False, ensemble_correlation=False,
          ensemble_families=False, ensemble_rank_diagnostics=False, **overrides):
    """Invert every sounding of the options file's data set.  One process per GPU: call from every rank of an initialised
    ``torch.distributed`` group to shard the soundings (``distributed.shard``); rank 0 returns the SurveyResult of the
    whole survey (and writes ``output`` if given), the other ranks return None.

    ``chunk``: soundings per block on the device (default 16 384 for "static" and "lines", fewer when full-length traces and hit maps of
    that many soundings would exceed BLOCK_PAYLOAD_BUDGET on the device; see "dynamic").
    ``schedule``: "auto" (the command line's default) -- "lines" on more than one rank when containers are written, the data file allows
    it and whole lines balance over the ranks (most loaded rank <= 1.2 x the mean), else "static";
    "lines" -- whole flight lines per rank, longest first to the least loaded rank (``distributed.assign_lines``): every
    rank writes the results containers of its own lines and no posterior row travels (the choice for many GPUs with containers);
    "static" -- each rank inverts one contiguous block (``distributed.shard``); "dynamic" -- the ranks draw chunks
    of ``chunk`` soundings (default: a 16th of a rank's static share, at least 256) from a shared counter until none are left
    (``distributed.ChunkQueue``; the reference's master / worker loop, Inference3D.py:518-635, without a master), which evens
    out the different numbers of iterations soundings need.  Chains are keyed by the sounding's row in the data file, so the
    results do not depend on the schedule.
    ``results_directory``: also write the reference's per-line results containers there (``<line number>.h5``: the layout of
    Inference2D.createHdf / Inference1D.writeHdf, ``geobipy_amd.hdf`` -- real HDF5 files, written by h5py when it is installed and through
    the HDF5 C library otherwise (``geobipy_amd.h5lite``); ``<line number>.results.npz`` with the same dataset paths where neither exists.
    ``container`` = "hdf5" | "npz" | None (the environment's GBP_CONTAINER, else whichever can be written; ``hdf.container_type()`` says
    which) -- every sounding's posteriors (layer count, interface depth, error levels, conductivity-depth hit
    map), best model and its predicted data.  The rows travel to rank 0 in bounded chunks (``distributed.stream_rows_to_root``).
    ``traces``: per-iteration misfit / acceptance traces for the containers' ``phids`` / ``acceptance_rate``, kept on the device at a stride --
    1 (default): the reference's arrays in full, 2 n_markov_chains columns, the shapes ``Inference1D.createHdf`` writes and its readers
    index by iteration; an int > 1 or "auto" (opt-in: the smallest stride with at most 4 096 entries per sounding): every stride-th
    entry side by side, ceil(2 n_markov_chains / stride) columns with the stride as the datasets' attribute ``trace_every`` -- NOT the
    reference's shapes; None: none.
    ``units`` (an interval spec, ``intervals.check_spec``: depth edges, elevation edges under the data file's elevations, horizons),
    ``unit_kinds``, ``first_above`` / ``first_below`` (S/m): the SAMPLED unit posteriors (``DeviceChains(units=...)``) -- the statistics of
    ``unit_posteriors.products`` are computed per block on the device and join the per-sounding summaries: ``unit_<kind>_*``,
    ``unit_conductance_*``, ``unit_resistance_*``, ``unit_thickness`` [S, M], ``first_depth_*``, ``first_probability`` [S, T] (statistics
    only: the histograms, 8 KB per kind and sounding, stay on the device).  Need the hit map.  The containers are not touched.
    ``data_posteriors`` (True or dict(n_bins, half_width, misfit_half_width)): the DATA-SPACE posteriors
    (``DeviceChains(data_posteriors=...)``) -- the statistics of ``data_posteriors.products`` join the per-sounding summaries the same
    way: ``data_residual_*``, ``data_predicted_*``, ``data_exceedance``, ``data_outside``, ``data_total`` [S, N] and ``misfit_median``,
    ``misfit_percentile_<p>``, ``misfit_share_below_one``, ``misfit_outside``, ``misfit_total`` [S].  Need the hit map too.
    ``ensemble`` (N or dict(n_keep, thin)): the POSTERIOR ENSEMBLE (``DeviceChains(ensemble=...)``; thin defaults to
    ceil(n_markov_chains / n_keep)) -- the kept models themselves join the per-sounding summaries: ``ensemble_k`` int32 [S, n_keep]
    (0: empty slot), ``ensemble_edges`` / ``ensemble_sigma`` [S, n_keep, K] (+inf / NaN padded), ``ensemble_misfit`` [S, n_keep] and
    ``ensemble_thin`` [S]; ``ensembles.realisations`` / ``ensembles.rebin`` take them from there.  Needs the hit map; counted in the
    default block's payload budget.  The containers are not touched.
    ``ensemble_diagnostics`` (True or dict(max_lag=1 .. 255); needs ``ensemble``): did the chains run long enough -- the chain
    diagnostics of the kept models (``ensembles.diagnostics``) join the summaries: ``ensemble_ess``, ``ensemble_rhat``
    (split R-hat: it works with one chain), ``ensemble_tau_iterations``, ``ensemble_mcse`` [S, n_depth] on the hit map's depth axis and
    ``ensemble_ess_k``, ``ensemble_ess_misfit``, ``ensemble_rhat_k``, ``ensemble_rhat_misfit``, ``ensemble_ess_min`` [S]; with
    ``replicates`` = C every chain of a sounding gives two segments.  The containers are not touched.
    ``ensemble_rank_diagnostics`` (True or dict(max_lag=1 .. 255, percentiles=(5, 50, 95)); needs ``ensemble``): did the chains run
    long enough for the percentiles -- the rank diagnostics of the kept models (``ensembles.rank_diagnostics``) join
    the summaries: ``ensemble_rhat_rank`` (the larger of the rank-normalised and the folded split R-hat), ``ensemble_ess_bulk`` and
    ``ensemble_ess_tail`` (the independent samples behind the lowest and the highest percentile) [S, n_depth], the same three with
    ``_k`` and ``_misfit`` [S] and ``ensemble_ess_bulk_min`` [S]; ``replicates`` = C as for the diagnostics.  The containers are not
    touched.
    ``ensemble_correlation`` (True or dict(band=64, threshold=0.5, keep_band=False); needs ``ensemble``): the vertical resolution -- the
    posterior correlation between depth cells of the kept models (``ensembles.correlation``) up to ``band`` cells apart:
    ``ensemble_resolution_length`` f64 (metres: the thickness of the run of cells whose correlation with the cell stays >= threshold),
    ``ensemble_resolution_cells`` int32 and ``ensemble_resolution_closed`` bool (False: the length is a lower bound) [S, n_depth] on the
    hit map's depth axis; with ``keep_band`` also ``ensemble_correlation_band`` [S, n_depth, W + 1].  ``replicates`` = C as for the
    diagnostics.  The containers are not touched.
    ``ensemble_families`` (True or dict(max_families=4, max_models=1024, measure="linear", min_silhouette=0.7); needs ``ensemble``): which
    kept model is representative, and is the posterior one family of models or several (``families.families``) on the
    window from the surface to the bottom of the hit map's depth axis: ``ensemble_central_k`` int32 [S], ``ensemble_central_edges`` /
    ``ensemble_central_sigma`` [S, K] and ``ensemble_central_mean_distance`` [S] (the medoid of the kept models: a sampled layered
    model, decades), ``ensemble_families_n`` int32 [S], ``ensemble_family_share`` and ``ensemble_family_silhouette`` [S, Q] (the shares
    of the selected stage's families, largest first; the silhouette of every stage), ``ensemble_family_k`` int32 [S, Q] and
    ``ensemble_family_edges`` / ``ensemble_family_sigma`` [S, Q, K] (the families' medoid models).  ``replicates`` = C as for the
    diagnostics.  The containers are not touched.
    ``replicates`` = C, 1 .. 8 (frequency-domain data): C chains per sounding that differ by their random streams alone
    (``replicates.expand``: replicate 0 walks the chain the sounding walks alone); a block then holds C rows per sounding and is seen
    through ``replicates.Pooled`` -- the containers and the posteriors of the summaries receive the sum over the chains that burned in,
    per-chain rows come from the chain with the highest posterior, and the summaries gain ``rhat``, ``jsd``, ``n_used`` [S, n_depth],
    ``chain_mean`` [S, C, n_depth], ``rhat_layers``, ``jsd_layers``, ``rhat_interfaces``, ``rhat_max`` and ``replicates_used`` [S]
    (DESIGN.md 3.15).  Needs the hit map.  1 (default): one chain per sounding, nothing changes.
    ``timings``: a dict that receives the wall time by phase (the device is synchronised at the phase borders then; bench.py).
    ``index`` / ``fiducial`` + ``line_number`` / ``line_number``: the reference's single-point and single-line switches.
    ``exact_jacobian``: use the true derivative of the forward model in the proposals instead of the reference's
    expression.  ``hankel_eps``: accuracy-budgeted window of the Hankel filter abscissae.  Frequency domain: ppm, per
    sounding, default 1e-10 (``DeviceChains(hankel_eps_ppm=...)``; 0 = all abscissae).  Time domain: relative to the
    inductive-limit value of every nodal sum, per sounding, default 1e-12 (``TdemDeviceChains(hankel_eps=...)``; 0 = all)."""
    import threading
    import torch
    import torch.distributed as dist
    from . import survey_run
    from .distributed import shard

    # check
    ens_diag = survey_run.ensemble_diagnostics_argument(ensemble_diagnostics, ensemble)
    ens_corr = survey_run.ensemble_correlation_argument(ensemble_correlation, ensemble)
    ens_fam = survey_run.ensemble_families_argument(ensemble_families, ensemble)
    ens_rank = survey_run.ensemble_rank_diagnostics_argument(ensemble_rank_diagnostics, ensemble)
    o = read_options(options, **overrides) if isinstance(options, str) else dict(options)
    tempest, time_domain, C_rep = survey_run.check_request(o, hitmap, replicates)
    # read
    if data is not None:
        ds = data
    elif time_domain:
        ds = (TempestData if tempest else TdemData).read_csv(o["data_filename"], o["system_filename"])
    else:
        ds = FdemData.read_csv(o["data_filename"], o["system_filename"])
    n_file = ds.nPoints
    rows = select_soundings(ds, index, fiducial, line_number)
    if rows.size != ds.nPoints:
        ds = ds.subset(rows)
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    start, n = shard(ds.nPoints, rank, world)
    # chains are keyed by the sounding's row in the data file, so a sounding inverted alone walks the chain it walks in the
    # full survey
    assert rows.size == 1 or np.all(np.diff(rows) == 1), "selected soundings must be contiguous rows"
    containers = results_directory is not None
    common = survey_run.sampler_arguments(o, time_domain, seed=seed, device=device, hitmap=hitmap, first_chain=int(rows[0]) + start,
                                          burn_in_min_iterations=burn_in_min_iterations, containers=containers, traces=traces,
                                          units=units is not None, unit_kinds=unit_kinds, first_above=first_above, first_below=first_below,
                                          data_posteriors=data_posteriors, hankel_eps=hankel_eps, ensemble=ensemble)
    ens_bytes = survey_run.ensemble_bytes(common["ensemble"]["n_keep"], o["maximum_number_of_layers"]) if "ensemble" in common else 0
    unit_z = None                                   # sampled unit posteriors: exact bounds of every sounding's units, metres below its
    if units is not None:                           # surface, cut at the end of the depth axis
        from .intervals import unit_bounds
        unit_z = unit_bounds(units, ds.nPoints, surface=ds.elevation, max_depth=1.1 * float(o["maximum_depth"]))
    # plan
    assert schedule in ("auto", "static", "dynamic", "lines"), ValueError("schedule must be 'auto', 'static', 'dynamic' or 'lines'")
    if schedule == "auto":
        schedule = survey_run.auto_schedule(ds.lineNumber, world, containers)
    block = lambda limit=16384: int(chunk) if chunk else survey_run.default_block(
        o["n_markov_chains"], common.get("trace_every"), hitmap and containers, C_rep, limit, ensemble_bytes=ens_bytes)
    # wall time by phase (device-synchronised at the phase borders only when a caller asks for it with timings={}: bench.py's
    # ``survey`` object; a normal run never synchronises for this)
    clock = survey_run.PhaseClock(timings)
    run = survey_run.SurveyRun(ds=ds, o=o, common=common, rows=rows, n_file=n_file, rank=rank, C_rep=C_rep,
                               time_domain=time_domain, hitmap=hitmap, exact_jacobian=exact_jacobian, check_every=check_every,
                               results_directory=results_directory, container=container,
                               own_containers=containers and (world == 1 or schedule == "lines"), unit_z=unit_z, clock=clock,
                               ensemble_diagnostics=ens_diag, ensemble_correlation=ens_corr, ensemble_families=ens_fam,
                               ensemble_rank_diagnostics=ens_rank)
    filler = survey_run.ContainerFiller(lambda dc, idx: run.payload(dc, idx, sparse=True),
                                        lambda dc: _LineWriter(results_directory, ds, o, dc, hitmap, container), clock)
    # the blocks, one after the other; a block's rows leave for the containers while the next block's chains run
    with filler:
        if schedule == "lines":
            # whole flight lines per rank: every rank fills and writes the results files of its own lines (as the reference's ranks
            # write their own rows, Inference3D.py:586-635), only the one-row summaries are gathered
            from .distributed import assign_lines
            firsts, counts, one_run_per_line = survey_run.line_runs(ds.lineNumber)
            if not one_run_per_line:
                raise ValueError("schedule='lines' needs every flight line in one run of consecutive rows of the data file (use 'static' or 'dynamic')")
            size = block()                          # a long line goes through the device in pieces of this many soundings
            ends = firsts + counts
            gathered = run.gather_pieces(((first, min(size, int(ends[li]) - first)) for li in assign_lines(counts, world)[rank]
                                          for first in range(int(firsts[li]), int(ends[li]), size)), filler)
        elif schedule == "static":
            # a rank's block goes through the device in pieces of `chunk` soundings (default 16 384): the posteriors of a piece (440 KB of
            # hit map per sounding) leave the GPU, and with one process the host, before the next piece runs -- 65 536 soundings: 19.6 s
            # and 16 GB of host memory in pieces against 24.7 s and 38 GB in one block (scripts/bench_survey.py); the chains are keyed by
            # row either way (a piece by every chain's own row, the whole shard by its first)
            piece = block()
            if n > piece:
                local = torch.cat([run.process(first, min(piece, start + n - first), filler) for first in range(start, start + n, piece)])
            else:
                local = run.process(start, n, filler, key_by_row=False)
            if world > 1:                           # the one exchange of the job: per-sounding result rows to rank 0
                from .distributed import SummaryGather
                g = SummaryGather(ds.nPoints, local.shape[1], local.device)
                gathered = g.finish(g.launch(*[local[:, i] for i in range(local.shape[1])]))
            else:
                gathered = local
        else:
            from .distributed import ChunkQueue
            gathered = run.gather_pieces(ChunkQueue(ds.nPoints, block(max(256, -(-ds.nPoints // (16 * world))))), filler)
    iterations_run = run.iterations
    if world > 1:                                   # an unfinished chain's count is the longest run of any rank
        it = torch.tensor([iterations_run], dtype=torch.int64, device=run.dc.device)
        dist.all_reduce(it, op=dist.ReduceOp.MAX)
        iterations_run = int(it)
    if rank != 0:
        run.write_containers(filler)
        return None
    with clock.phase("summaries_to_host"):
        r = gathered.cpu().numpy()
    # the result is put together and the summary file compressed on a thread of its own while this one fills the line containers and
    # their writer threads finish (numpy's conversions and zlib release the interpreter lock)
    failed, made = [], []

    def assemble_and_save():
        try:
            made.append(survey_run.assemble_result(ds, o, run.dc, run.named, r, iterations_run))
            if output is not None:
                made[0].save(output)
        except BaseException as e:                       # (handed to the caller's thread below)
            failed.append(e)
    saver = threading.Thread(target=assemble_and_save)
    saver.start()
    try:
        run.write_containers(filler)
    finally:
        with clock.phase("summary_file_tail"):
            saver.join()
    if failed:
        raise failed[0]
    return made[0]
