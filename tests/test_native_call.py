"""The one path from a product module to a ``gbp_*`` entry (``_lib.pointers`` / ``_lib.call``) and the checks the products share
(``_args``), on the host: the marshalling rules, the refusals of tensors a kernel would read wrongly, the call against a recording
fake of the library, and the texts the product modules' own tests match, for both owning modules."""
import contextlib
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

from geobipy_amd import _args, _lib

CPU = torch.device("cpu")
Ens = namedtuple("Ens", ("k", "edges", "sigma", "misfit"))


def test_pointers_marshal_tensors_and_pass_the_rest_through():
    t, e = torch.arange(6, dtype=torch.float64), torch.empty((0, 3), dtype=torch.int32)
    arr, handle, ref = (ctypes.c_double * 3)(1.0, 2.0, 3.0), ctypes.c_void_p(77), ctypes.byref(ctypes.c_void_p())
    args = (t, None, 3, 2.5, arr, handle, ref, e)
    out = _lib.pointers("gbp_x", CPU, args)
    assert out[0] == t.data_ptr() and out[1] is None and out[7] == e.data_ptr()
    for i in range(2, 7):
        assert out[i] is args[i]
    assert type(out[2]) is int and type(out[3]) is float
    assert _lib.pointers("gbp_x", CPU, ()) == []


def test_pointers_refuse_what_a_kernel_would_read_wrongly():
    t = torch.zeros((4, 3, 2))
    for bad, position, word in ((torch.zeros((2, 3)).t(), 1, "contiguous"), (t[:, 1], 1, "contiguous"),
                                (torch.zeros(3, device="meta"), 1, "meta"), (torch.zeros((2, 3)).t(), 2, "contiguous")):
        args = (5,) * position + (bad,)
        with pytest.raises(_lib.NativeLibraryError, match=r"gbp_some_entry: argument %d .*%s" % (position, word)):
            _lib.pointers("gbp_some_entry", CPU, args)
    with pytest.raises(_lib.NativeLibraryError, match="gbp_some_entry: argument 0 .*cpu"):
        _lib.pointers("gbp_some_entry", torch.device("meta"), (torch.zeros(3),))


def test_pointers_accept_the_slices_the_modules_pass():
    t, v = torch.zeros((4, 3, 2)), torch.zeros(5, dtype=torch.int64)
    step = t.element_size()
    out = _lib.pointers("gbp_x", CPU, (t[1:3], t[0], v[1:], t[2:2]))
    assert out[0] == t.data_ptr() + 6 * step and out[1] == t.data_ptr() and out[2] == v.data_ptr() + 8


class _FakeLibrary:
    """Records the calls of one entry, ``gbp_fake``, and answers with ``status``."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def gbp_fake(self, *args):
        self.calls.append(args)
        return self.status

    def gbp_last_error(self):
        return b"the fake failed"


def _patch(monkeypatch, lib):
    entered = []

    @contextlib.contextmanager
    def device(dev):
        entered.append(dev)
        yield

    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "stream", lambda dev: 4242)
    monkeypatch.setattr(torch.cuda, "device", device)
    return entered


def test_call_marshals_appends_the_stream_and_checks_the_status(monkeypatch):
    lib = _FakeLibrary()
    entered = _patch(monkeypatch, lib)
    t, arr = torch.zeros((2, 3), dtype=torch.float64), (ctypes.c_double * 3)()
    _lib.call("gbp_fake", CPU, 2, t, None, 0.5, arr, t[1])
    assert lib.calls == [(2, t.data_ptr(), None, 0.5, arr, t.data_ptr() + 24, 4242)] and entered == [CPU]
    _lib.call("gbp_fake", CPU)
    assert lib.calls[1] == (4242,)

    failing = _FakeLibrary(status=3)
    _patch(monkeypatch, failing)
    with pytest.raises(_lib.NativeLibraryError, match=r"status 3\): the fake failed"):
        _lib.call("gbp_fake", CPU, 1, t)
    assert len(failing.calls) == 1

    with pytest.raises(AttributeError):                      # an entry the library does not have is an error, never a fallback
        _lib.call("gbp_missing", CPU, 1)


def test_call_refuses_before_the_entry_and_before_the_library(monkeypatch):
    lib = _FakeLibrary()
    entered = _patch(monkeypatch, lib)
    for bad in (torch.zeros((2, 3)).t(), torch.zeros(3, device="meta")):
        with pytest.raises(_lib.NativeLibraryError, match="gbp_fake: argument 1"):
            _lib.call("gbp_fake", CPU, 1, bad)
    assert lib.calls == [] and entered == []
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    with pytest.raises(_lib.NativeLibraryError, match="gbp_fake: argument 0"):
        _lib.call("gbp_fake", CPU, torch.zeros((2, 3)).t())


@pytest.mark.parametrize("prefix", ["sections", "horizons"])
def test_check_ptr_texts_for_both_modules(prefix):
    for bad, match in ((np.zeros((2, 2)), "vector"), (np.array([0.0, 3.0]), "vector"), ([1, 3], "start at 0"), ([0, 2], "end at"),
                       ([0, 1, 1, 3], "at least one"), ([0, 2, 2, 3], "at least one")):
        with pytest.raises(ValueError, match="^%s: ptr must .*%s" % (prefix, match)):
            _args.check_ptr(bad, 3, prefix)
    with pytest.raises(ValueError, match=r"^%s: ptr must be a vector of L \+ 1 integers$" % prefix):
        _args.check_ptr([], 0, prefix)
    with pytest.raises(ValueError, match=r"^%s: ptr must start at 0, end at the number of soundings \(3\) and give every sequence at least one$" % prefix):
        _args.check_ptr([0, 1, 1, 3], 3, prefix)
    with pytest.raises(ValueError, match=r"^%s: ptr must start at 0, end at the number of soundings \(3\) and not decrease$" % prefix):
        _args.check_ptr([0, 2, 1, 3], 3, prefix, empty=True)
    p = _args.check_ptr(torch.tensor([0, 1, 3], dtype=torch.int32), 3, prefix)
    assert p.dtype == np.int64 and p.tolist() == [0, 1, 3]
    assert _args.check_ptr([0, 1, 1, 3], 3, prefix, empty=True).tolist() == [0, 1, 1, 3]
    assert _args.check_ptr([0], 0, prefix, empty=True).tolist() == [0]


def test_the_modules_check_ptr_are_the_shared_one():
    from geobipy_amd import horizons, sections
    for module, prefix in ((sections, "sections"), (horizons, "horizons")):
        with pytest.raises(ValueError, match="^%s: ptr must start at 0" % prefix):
            module.check_ptr([1, 3], 3)
        assert module.check_ptr([0, 3], 3).tolist() == [0, 3]
    assert sections.check_ptr([0, 0, 3], 3, empty=True).tolist() == [0, 0, 3]


def _ensemble(B=2, ns=4, K=3):
    return Ens(torch.ones((B, ns), dtype=torch.int32), torch.zeros((B, ns, K), dtype=torch.float64), torch.ones((B, ns, K), dtype=torch.float64),
               torch.ones((B, ns), dtype=torch.float64))


@pytest.mark.parametrize("batch, slots", [("B", "n_slots"), ("S", "n_slots"), ("B", "n_keep")])
def test_check_ensemble_shapes_dtypes_and_texts(batch, slots):
    ens = _ensemble()
    k, edges, sigma, B, ns, K = _args.check_ensemble(ens, batch=batch, slots=slots)
    assert (B, ns, K) == (2, 4, 3) and k.is_contiguous() and edges.is_contiguous() and sigma.is_contiguous()
    text = r"^ensemble: k \[%s, %s\], edges and sigma \[%s, %s, K\]$" % (batch, slots, batch, slots)
    for bad in (dict(k=ens.k[:, :3]), dict(k=ens.k[0]), dict(edges=ens.edges[:, :, :2]), dict(sigma=ens.sigma[0]), dict(edges=ens.edges[:1], sigma=ens.sigma[:1])):
        with pytest.raises(ValueError, match=text):
            _args.check_ensemble(ens._replace(**bad), batch=batch, slots=slots)
    for bad in (dict(k=ens.k.long()), dict(edges=ens.edges.float(), sigma=ens.sigma.float()), dict(sigma=ens.sigma.float())):
        with pytest.raises(TypeError, match="^ensemble: k is int32, edges and sigma are float64$"):
            _args.check_ensemble(ens._replace(**bad), batch=batch, slots=slots)
    # a transposed ensemble comes back contiguous, the values untouched
    turned = ens._replace(edges=ens.edges.permute(0, 2, 1).contiguous().permute(0, 2, 1))
    assert not turned.edges.is_contiguous() and _args.check_ensemble(turned)[1].is_contiguous()


def test_check_ensemble_misfit_and_rows_keep_their_place_in_the_order():
    ens = _ensemble()
    with pytest.raises(ValueError, match=r"^ensemble: k and misfit \[B, n_slots\], edges and sigma \[B, n_slots, K\]$"):
        _args.check_ensemble(ens._replace(misfit=ens.misfit[:, :3]), misfit=True)
    with pytest.raises(TypeError, match="^ensemble: k is int32, edges and sigma are float64, misfit is floating point$"):
        _args.check_ensemble(ens._replace(misfit=ens.k), misfit=True)
    _args.check_ensemble(ens._replace(misfit=ens.misfit.float()), misfit=True)
    _args.check_ensemble(ens._replace(misfit=None))                       # misfit takes no part: it is not looked at

    rows = torch.zeros((2, 5), dtype=torch.int32)
    kw = dict(batch="S", what="cross_distance", max_rows=4096)
    assert _args.check_ensemble(ens, rows=rows, **kw)[3:] == (2, 4, 3)
    for bad in (rows[0], rows[:1], torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 4097), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"^cross_distance: rows \[S, n\] with 1 <= n <= 4096$"):
            _args.check_ensemble(ens, rows=bad, **kw)
    with pytest.raises(TypeError, match="^ensemble: k is int32, edges and sigma are float64; rows is int32$"):
        _args.check_ensemble(ens, rows=rows.long(), **kw)
    # the order: the ensemble's shapes, the rows' shape, then every dtype
    with pytest.raises(ValueError, match="^ensemble: k"):
        _args.check_ensemble(ens._replace(k=ens.k[:, :3].long()), rows=rows[0], **kw)
    with pytest.raises(ValueError, match="^cross_distance: rows"):
        _args.check_ensemble(ens._replace(k=ens.k.long()), rows=rows[0], **kw)
    with pytest.raises(ValueError, match=r"^distance: rows \[B, n\] with 1 <= n <= 8$"):
        _args.check_ensemble(ens, rows=torch.zeros((2, 9), dtype=torch.int32), what="distance", max_rows=8)


def test_check_block_and_check_int():
    for ok in (None, 1, 7, np.int64(3), 2.0):
        _args.check_block(ok, "distance")
    for bad in (0, -1, True, 1.5):
        with pytest.raises(ValueError, match="^cross_distance: block must be a positive integer$"):
            _args.check_block(bad, "cross_distance")
    assert _args.check_int(3, 1, 8, "max_families") == 3 and type(_args.check_int(np.int32(8), 1, 8, "--chains")) is int
    for bad in (0, 9, True, 2.0, "3", None):
        with pytest.raises(ValueError, match=r"^sections.draw: n_draws must be an integer in 1 \.\. 8$"):
            _args.check_int(bad, 1, 8, "sections.draw: n_draws")


def test_device_checks_name_the_module_the_entry_and_the_kernel():
    t = torch.zeros(2)
    for module in ("ensembles", "families", "sections"):
        with pytest.raises(_lib.NativeLibraryError, match=r"^%s.track takes torch tensors on the device \(gbp_x\); there is no host fallback$" % module):
            _args.are_tensors((t, np.zeros(2)), module, "track", "gbp_x")
        with pytest.raises(_lib.NativeLibraryError, match=r"^%s.track runs on the device \(gbp_x\); there is no host fallback$" % module):
            _args.on_device((t,), module, "track", "gbp_x")
        _args.are_tensors((t,), module, "track", "gbp_x")
    _args.on_device((), "sections", "track", "gbp_x")


def test_first_max_is_the_one_lane_loop():
    def loop(v):
        cur = 0
        for j in range(1, v.size):
            if v[j] > v[cur]:
                cur = j
        return cur

    rng = np.random.default_rng(3)
    nan, inf = np.nan, np.inf
    cases = [np.array(v) for v in ([1.0], [2.0, 2.0], [1.0, 3.0, 3.0, 2.0], [-inf, -inf], [nan, 1.0], [1.0, nan, 2.0, nan, 2.0], [nan, nan], [-inf, nan, -inf],
                                   [inf, nan, inf])]
    cases += [rng.integers(0, 4, n).astype(np.float64) for n in (2, 5, 33)]
    cases += [np.where(rng.random(9) < 0.3, nan, rng.integers(0, 3, 9)).astype(dt) for dt in (np.float64, np.longdouble) for _ in range(8)]
    for v in cases:
        assert _args.first_max(v) == loop(v), v


def test_save_npz_and_load_npz_round_trip(tmp_path):
    result = dict(a=torch.arange(3, dtype=torch.int32), b=np.array([[1.5, np.nan]]), c=2.5, d=torch.ones(2, requires_grad=True))
    path = _args.save_npz(result, str(tmp_path / "r.npz"))
    back = _args.load_npz(path)
    assert set(back) == set(result) and back["a"].dtype == np.int32 and back["a"].tolist() == [0, 1, 2]
    assert np.array_equal(back["b"], result["b"], equal_nan=True) and float(back["c"]) == 2.5 and back["d"].tolist() == [1.0, 1.0]
    from geobipy_amd import data_posteriors, horizons, sections, unit_posteriors
    for module in (horizons, sections, unit_posteriors, data_posteriors):
        assert module.save is _args.save_npz
    for module in (horizons, sections, data_posteriors):
        assert module.load is _args.load_npz
