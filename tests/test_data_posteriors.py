"""Data-space posteriors, CPU tier: the host rule (inference.Posteriors(data=...): residual of every channel's prediction, misfit), the
elementwise statistics of data_posteriors on CPU tensors, and the sampler's refusals before it touches the device.  The device
accumulators are held against this host rule in tests/test_data_posteriors_gpu.py."""
import math

import numpy as np
import pytest
import torch

from geobipy_amd import data_posteriors
from geobipy_amd.inference import Posteriors


def _posteriors(observed, scale, **kw):
    return Posteriors(30, 150.0, 1.0, 0.05, data=dict(observed=observed, scale=scale, **kw))


def test_hand_made_predictions_land_in_the_cells_computed_by_hand():
    # 64 cells on +-8: cell width 0.25, pos = (r + 8) * 4
    residuals = [-8.5, -8.0, -0.125, 0.1, 7.99, 8.0, 9.0]
    cells = [0, 0, 31, 32, 63, 63, 63]                            # -8.5 and 9 (and 8 itself, pos = 64) are clamped to the end cells
    assert [int(min(max(math.floor((r + 8.0) * 4.0), 0), 63)) for r in residuals] == cells
    obs = np.array([100.0, 250.0, 40.0])
    scale = np.array([2.0, 0.5, 4.0])                             # (powers of two: obs + r scale and back are exact)
    p = _posteriors(obs, scale, n_bins=64, half_width=8.0)
    assert p.data_hist.shape == (64, 3) and p.data_hist.dtype == np.int64 and p.misfit_hist.shape == (64,)
    for r in residuals:
        p.update(np.zeros(0), np.array([0.1]), predicted=obs + r * scale, misfit=3.0)
    want = np.zeros((64, 3), dtype=np.int64)
    for c in cells:
        want[c, :] += 1
    assert np.array_equal(p.data_hist, want)
    assert p.data_hist[0, 0] == 2 and p.data_hist[63, 0] == 3     # the clamped ones sit in the end cells
    assert np.array_equal(p.data_hist.sum(axis=0), [len(residuals)] * 3) and p.misfit_hist.sum() == len(residuals)
    p.reset()
    assert p.data_hist.sum() == 0 and p.misfit_hist.sum() == 0 and p.misfit_edge_distance == []


def test_inactive_channels_and_non_finite_predictions_get_nothing():
    obs = np.array([100.0, 0.0, -5.0, np.nan, 30.0])              # the sampler's active rule: obs > 0
    p = _posteriors(obs, np.full(5, 2.0), n_bins=64, half_width=8.0)
    assert p.misfit_scale == 2.0                                  # the number of active channels
    n = 0
    for pred in (obs + 1.0, np.array([101.0, 5.0, 5.0, 5.0, np.nan]), np.array([np.inf, 1.0, 1.0, 1.0, 29.0]),
                 np.array([-np.inf, 1.0, 1.0, 1.0, 31.0])):
        p.update(np.zeros(0), np.array([0.1]), predicted=pred, misfit=2.0)
        n += 1
    per_channel = p.data_hist.sum(axis=0)
    assert np.array_equal(per_channel[1:4], [0, 0, 0])            # inactive: nothing
    assert per_channel[0] == 2 and per_channel[4] == 3            # +-inf and NaN predictions go to no cell (not to the end cells)
    assert p.data_hist[0].sum() == 0 and p.data_hist[63].sum() == 0
    assert p.misfit_hist.sum() == n
    # the sum over the cells is the number of updates on active channels with a finite prediction
    q = _posteriors(obs, np.full(5, 2.0))
    for _ in range(9):
        q.update(np.zeros(0), np.array([0.1]), predicted=np.where(obs > 0, obs, 1.0), misfit=2.0)
    assert np.array_equal(q.data_hist.sum(axis=0), [9, 0, 0, 0, 9]) and q.data_hist.shape == (64, 5)      # (defaults: 64 cells)
    # a non-finite or zero misfit goes to no cell either
    q.update(np.zeros(0), np.array([0.1]), misfit=np.nan)
    q.update(np.zeros(0), np.array([0.1]), misfit=0.0)
    assert q.misfit_hist.sum() == 9


def test_misfit_cells_at_two_decades():
    # 64 cells on +-2 decades: 16 cells per decade, pos = (log10(chi^2 / N) + 2) * 16
    N = 4
    p = _posteriors(np.full(N, 10.0), np.ones(N), n_bins=64, half_width=8.0, misfit_half_width=2.0)
    cases = [(0.005, 0), (0.01, 0), (1.0, 32), (3.0, int(math.floor((math.log10(3.0) + 2.0) * 16.0))), (250.0, 63)]
    assert cases[3][1] == 39
    for ratio, cell in cases:
        before = p.misfit_hist.copy()
        p.update(np.zeros(0), np.array([0.1]), misfit=ratio * N)
        got = np.nonzero(p.misfit_hist - before)[0]
        if ratio in (0.01, 1.0):                                  # exactly on a cell edge: the last bit of the logarithm decides
            assert got.size == 1 and abs(int(got[0]) - cell) <= 1 and p.misfit_edge_distance[-1] < 1e-9, ratio
        else:
            assert np.array_equal(got, [cell]), ratio
            assert p.misfit_edge_distance[-1] > 1e-3 or ratio in (0.005, 250.0)
    assert p.misfit_hist.sum() == 5 and len(p.misfit_edge_distance) == 5
    assert p.data_hist.sum() == 0                                 # no prediction given: the residual histograms are untouched


def test_bad_data_arguments_are_refused():
    obs = np.array([1.0, 2.0])
    for kw in (dict(n_bins=7), dict(n_bins=257), dict(n_bins=12.5), dict(half_width=0.0), dict(half_width=-1.0), dict(half_width=np.nan),
               dict(misfit_half_width=0.0), dict(misfit_half_width=np.inf)):
        with pytest.raises(ValueError):
            _posteriors(obs, np.ones(2), **kw)
    with pytest.raises(ValueError):
        _posteriors(obs, np.array([1.0, 0.0]))                    # the scale of an active channel must be positive
    _posteriors(np.array([1.0, 0.0]), np.array([1.0, 0.0]))       # ... of an inactive one it does not matter
    off = Posteriors(30, 150.0, 1.0, 0.05)
    off.update(np.zeros(0), np.array([0.1]), predicted=np.ones(2), misfit=1.0)           # feature off: ignored
    assert off.data_hist.size == 0 and off.misfit_hist.size == 0


def test_exceedance_and_outside_shares_on_cpu_tensors():
    # even axis: 8 cells, centres -3.5 ... 3.5 -- cells 4 .. 7 are above 0
    h = torch.zeros((2, 8, 3), dtype=torch.int32)
    h[0, :, 0] = torch.tensor([1, 0, 2, 3, 4, 0, 5, 5])           # 20 samples, 14 above, 6 in the end cells
    h[0, 2, 1] = 9                                                # all below
    h[1, 7, 0] = 4                                                # all in the upper end cell
    out = data_posteriors.shares(h)
    assert out["data_total"].dtype == torch.int64 and np.array_equal(out["data_total"].numpy(), [[20, 9, 0], [4, 0, 0]])
    ex, outside = out["data_exceedance"].numpy(), out["data_outside"].numpy()
    assert ex[0, 0] == 14 / 20 and ex[0, 1] == 0.0 and ex[1, 0] == 1.0
    assert outside[0, 0] == 6 / 20 and outside[0, 1] == 0.0 and outside[1, 0] == 1.0
    assert np.isnan(ex[0, 2]) and np.isnan(ex[1, 1:]).all() and np.isnan(outside[0, 2])          # an empty column: NaN
    # odd axis: 9 cells, cell 4 is centred on 0 and counts half
    h = torch.zeros((1, 9, 2), dtype=torch.int64)
    h[0, :, 0] = torch.tensor([2, 0, 0, 1, 6, 3, 0, 0, 4])        # 16 samples: 7 above + half of 6
    h[0, 4, 1] = 5                                                # all on the centre cell
    out = data_posteriors.shares(h)
    assert out["data_exceedance"].numpy()[0, 0] == (7 + 3) / 16 and out["data_exceedance"].numpy()[0, 1] == 0.5
    assert out["data_outside"].numpy()[0, 0] == 6 / 16


def test_misfit_statistics_on_cpu_tensors():
    nb, hw = 64, 2.0
    centre = lambda i: 10.0 ** ((i + 0.5) * (2 * hw / nb) - hw)      # noqa: E731
    mh = torch.zeros((4, nb), dtype=torch.int32)
    mh[0, 20] = 30; mh[0, 40] = 70                                # 30 % at cell 20, 70 % at cell 40
    mh[1, 0] = 5; mh[1, 63] = 15                                  # everything outside
    mh[2, 31] = 8                                                 # all just below chi^2 / N = 1
    out = data_posteriors.misfit_statistics(mh, hw, (5, 50, 95))
    for k in ("misfit_median", "misfit_percentile_5", "misfit_percentile_50", "misfit_percentile_95", "misfit_share_below_one",
              "misfit_outside", "misfit_total"):
        assert out[k].shape == (4,), k
    med, p5, p95 = out["misfit_median"].numpy(), out["misfit_percentile_5"].numpy(), out["misfit_percentile_95"].numpy()
    assert np.allclose([med[0], p5[0], p95[0]], [centre(40), centre(20), centre(40)], rtol=1e-14)
    assert np.array_equal(out["misfit_percentile_50"].numpy(), med, equal_nan=True)
    assert np.allclose([med[1], p5[1], med[2]], [centre(63), centre(0), centre(31)], rtol=1e-14)
    below, outside = out["misfit_share_below_one"].numpy(), out["misfit_outside"].numpy()
    assert below[0] == 0.3 and below[1] == 0.25 and below[2] == 1.0
    assert outside[0] == 0.0 and outside[1] == 1.0 and outside[2] == 0.0
    for k in ("misfit_median", "misfit_percentile_5", "misfit_share_below_one", "misfit_outside"):
        assert np.isnan(out[k].numpy()[3]), k                     # no samples: NaN
    assert np.array_equal(out["misfit_total"].numpy(), [100, 20, 8, 0])
    odd = torch.zeros((1, 9), dtype=torch.int32)
    odd[0, 4] = 6; odd[0, 1] = 2                                  # the centre cell counts half
    assert data_posteriors.misfit_statistics(odd, hw)["misfit_share_below_one"].numpy()[0] == (2 + 3) / 8


def test_save_and_load_round_trip(tmp_path):
    h = torch.zeros((1, 8, 2), dtype=torch.int32)
    h[0, 5, 0] = 3
    out = dict(data_posteriors.shares(h), misfit_median=np.array([1.5]))
    path = data_posteriors.save(out, str(tmp_path / "data.npz"))
    back = data_posteriors.load(path)
    assert set(back) == set(out)
    assert np.array_equal(back["data_exceedance"], out["data_exceedance"].numpy(), equal_nan=True)
    assert np.array_equal(back["data_total"], [[3, 0]]) and np.array_equal(back["misfit_median"], [1.5])


def test_sampler_refuses_bad_data_arguments_before_touching_the_device():
    """DeviceChains(data_posteriors=...) checks its arguments with the host rule's checks, before the first device call: no hit map,
    ignore_likelihood, bins out of range, a width that is not positive and finite."""
    from geobipy_amd import rjmcmc_gpu
    from geobipy_amd.inference import check_data_posteriors, data_posteriors_argument
    assert data_posteriors_argument(None) is None and data_posteriors_argument(False) is None
    assert data_posteriors_argument(True) == dict(n_bins=64, half_width=8.0, misfit_half_width=2.0, scale=None)
    assert data_posteriors_argument(dict(n_bins=32, half_width=4))["n_bins"] == 32
    for bad in (dict(n_bins=7), dict(n_bins=257), dict(half_width=0.0), dict(half_width=-2.0), dict(misfit_half_width=float("nan")),
                dict(misfit_half_width=0.0), dict(bins=64)):
        with pytest.raises(ValueError):
            data_posteriors_argument(bad)
    assert check_data_posteriors(8, 1.0, 1.0) == (8, 1.0, 1.0) and check_data_posteriors(256, 1.0, 1.0)[0] == 256

    class NoDevice:
        """Stands where the system handle would: any use is a device call the refusal must come before."""
        def __getattr__(self, name):
            raise AssertionError("the sampler touched the system (%s) before refusing its arguments" % name)

    opts = dict(maximum_number_of_layers=12, minimum_depth=1.0, maximum_depth=150.0, minimum_thickness=1.0, initial_relative_error=0.05,
                minimum_relative_error=0.001, maximum_relative_error=0.5, initial_additive_error=5.0, minimum_additive_error=3.0,
                maximum_additive_error=20.0, relative_error_proposal_variance=1e-6, additive_error_proposal_variance=1e-6,
                probability_of_birth=1 / 6, probability_of_death=1 / 6, probability_of_perturb=1 / 6, probability_of_no_change=0.5)
    heights, data = np.full(2, 30.0), np.full((2, 12), 100.0)
    make = lambda **kw: rjmcmc_gpu.DeviceChains(NoDevice(), heights, data, device="cpu", hankel_eps_ppm=0.0, **kw, **opts)      # noqa: E731
    with pytest.raises(ValueError, match="hitmap"):
        make(data_posteriors=True)                                # no hit map
    with pytest.raises(ValueError, match="ignore_likelihood"):
        make(hitmap=True, ignore_likelihood=True, data_posteriors=True)
    for bad in (dict(n_bins=7), dict(n_bins=257), dict(half_width=0.0), dict(misfit_half_width=-1.0)):
        with pytest.raises(ValueError, match="data posteriors"):
            make(hitmap=True, data_posteriors=bad)
    with pytest.raises(ValueError, match="scale"):
        make(hitmap=True, data_posteriors=dict(scale=np.ones((3, 12))))
