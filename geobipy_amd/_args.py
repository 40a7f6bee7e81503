"""The argument checks and small helpers the posterior product modules share: one definition each, with the owning module's name or
prefix as a parameter where the message carries it.  A product refuses in the order tensors, shapes, dtypes, values and the device
last, and never loads the library before a refusal; the launch itself goes through ``_lib.call``."""
import numpy as np
import torch

from ._lib import NativeLibraryError


def are_tensors(tensors, module, what, entry):
    for a in tensors:
        if not torch.is_tensor(a):
            raise NativeLibraryError("%s.%s takes torch tensors on the device (%s); there is no host fallback" % (module, what, entry))


def on_device(tensors, module, what, entry):
    """The last check of an entry: shapes, dtypes and values are refused first, whatever device the tensors are on."""
    for a in tensors:
        if a.device.type != "cuda":
            raise NativeLibraryError("%s.%s runs on the device (%s); there is no host fallback" % (module, what, entry))


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def check_block(block, what):
    if block is not None and (isinstance(block, bool) or int(block) != block or int(block) < 1):
        raise ValueError("%s: block must be a positive integer" % what)


def check_int(value, lo, hi, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError("%s must be an integer in %d .. %d" % (what, lo, hi))
    return int(value)


def check_ptr(ptr, total, prefix, empty=False):
    """``ptr`` (host or torch) as int64 numpy [L + 1]: starts at 0, ends at ``total``, every sequence holds at least one sounding
    (``empty``: or none).  ``prefix``: the module the message names."""
    p = np.asarray(ptr.cpu() if torch.is_tensor(ptr) else ptr)
    if p.ndim != 1 or p.size < 1 or p.dtype.kind not in "iu":
        raise ValueError("%s: ptr must be a vector of L + 1 integers" % prefix)
    p = p.astype(np.int64)
    if empty and (p[0] != 0 or p[-1] != total or np.any(np.diff(p) < 0)):
        raise ValueError("%s: ptr must start at 0, end at the number of soundings (%d) and not decrease" % (prefix, total))
    if p[0] != 0 or p[-1] != total or (not empty and np.any(np.diff(p) < 1)):
        raise ValueError("%s: ptr must start at 0, end at the number of soundings (%d) and give every sequence at least one" % (prefix, total))
    return p


def first_max(v):
    """The first maximum of a vector with strict > to replace, starting from v[0] (what the device's one lane does): a NaN never
    replaces, and a NaN at v[0] is never replaced."""
    return 0 if v[0] != v[0] else int(np.nanargmax(v))


def check_ensemble(ens, batch="B", slots="n_slots", misfit=False, rows=None, what=None, max_rows=None):
    """The shapes and dtypes of an ensemble's tensors (any device): k int32 [B, n_slots], edges and sigma float64 [B, n_slots, K];
    ``misfit``: it takes part, floating point [B, n_slots]; ``rows``: the entry ``what`` also takes model lists int32 [B, n] with
    1 <= n <= ``max_rows``.  ``batch`` / ``slots``: the caller's names of the axes in the text.  Returns k, edges, sigma
    (contiguous), B, n_slots, K; the caller's own size limits come after."""
    k, edges, sigma = ens.k, ens.edges, ens.sigma
    if k.ndim != 2 or edges.ndim != 3 or edges.shape != sigma.shape or tuple(edges.shape[:2]) != tuple(k.shape) or (misfit and ens.misfit.shape != k.shape):
        raise ValueError("ensemble: %s [%s, %s], edges and sigma [%s, %s, K]" % ("k and misfit" if misfit else "k", batch, slots, batch, slots))
    if rows is not None and (rows.ndim != 2 or rows.shape[0] != k.shape[0] or not 1 <= rows.shape[1] <= max_rows):
        raise ValueError("%s: rows [%s, n] with 1 <= n <= %d" % (what, batch, max_rows))
    if k.dtype != torch.int32 or edges.dtype != torch.float64 or sigma.dtype != torch.float64 or (misfit and not ens.misfit.dtype.is_floating_point) \
            or (rows is not None and rows.dtype != torch.int32):
        raise TypeError("ensemble: k is int32, edges and sigma are float64" + (", misfit is floating point" if misfit else "")
                        + ("; rows is int32" if rows is not None else ""))
    B, ns, K = edges.shape
    return k.contiguous(), edges.contiguous(), sigma.contiguous(), B, ns, K


def save_npz(result, path):
    """Write a result ({name: tensor or array}) to ``path`` with np.savez_compressed; returns the path."""
    np.savez_compressed(path, **{k: host(v) for k, v in result.items()})
    return path


def load_npz(path):
    """{name: numpy array} of a file written by ``save_npz``."""
    with np.load(path) as f:
        return {k: f[k] for k in f.files}
