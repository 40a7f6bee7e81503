"""Every key of the SurveyResult keeps its dtype and shape: survey.infer with every per-sounding product on at its smallest setting, eight
soundings in three blocks (chunk=3: the last one ragged, so the blocks' layouts must agree), against the table of the commit before
the summaries carried their own layout (the same call there printed it)."""
import os

import numpy as np
import pytest

from geobipy_amd import survey

pytestmark = pytest.mark.gpu

OPTIONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resolve_options_small")
SHORT = dict(n_markov_chains=400, burn_in_min_iterations=150, check_every=100, exact_jacobian=True, chunk=3)

ALL_PRODUCTS = {
    'line': ('float64', (8,)), 'fiducial': ('float64', (8,)), 'x': ('float64', (8,)), 'y': ('float64', (8,)), 'z': ('float64', (8,)), 'elevation': ('float64',
    (8,)), 'depth_bin_width': ('float64', ()), 'status': ('int32', (8,)), 'burned_in_iteration': ('int32', (8,)), 'misfit': ('float64', (8,)), 'relative_error':
    ('float64', (8,)), 'additive_error': ('float64', (8,)), 'n_layers': ('int32', (8,)), 'best_n_layers': ('int32', (8,)), 'best_posterior': ('float64', (8,)),
    'best_edges': ('float64', (8, 30)), 'best_conductivity': ('float64', (8, 30)), 'layer_count_posterior': ('int64', (8, 31)), 'interface_posterior': ('int64',
    (8, 440)), 'relative_error_posterior': ('int64', (8, 99)), 'additive_error_posterior': ('int64', (8, 99)), 'mean_log10_conductivity': ('float64', (8, 440)),
    'log10_conductivity_p05': ('float64', (8, 440)), 'log10_conductivity_p50': ('float64', (8, 440)), 'log10_conductivity_p95': ('float64', (8, 440)),
    'unit_arithmetic_mean': ('float64', (8, 3)), 'unit_arithmetic_median': ('float64', (8, 3)), 'unit_arithmetic_mode': ('float64', (8, 3)),
    'unit_arithmetic_credible_range': ('float64', (8, 3)), 'unit_arithmetic_percentile_5': ('float64', (8, 3)), 'unit_arithmetic_percentile_50': ('float64', (8,
    3)), 'unit_arithmetic_percentile_95': ('float64', (8, 3)), 'unit_conductance_mean': ('float64', (8, 3)), 'unit_conductance_median': ('float64', (8, 3)),
    'unit_conductance_mode': ('float64', (8, 3)), 'unit_conductance_credible_range': ('float64', (8, 3)), 'unit_conductance_percentile_5': ('float64', (8, 3)),
    'unit_conductance_percentile_50': ('float64', (8, 3)), 'unit_conductance_percentile_95': ('float64', (8, 3)), 'unit_harmonic_mean': ('float64', (8, 3)),
    'unit_harmonic_median': ('float64', (8, 3)), 'unit_harmonic_mode': ('float64', (8, 3)), 'unit_harmonic_credible_range': ('float64', (8, 3)),
    'unit_harmonic_percentile_5': ('float64', (8, 3)), 'unit_harmonic_percentile_50': ('float64', (8, 3)), 'unit_harmonic_percentile_95': ('float64', (8, 3)),
    'unit_resistance_mean': ('float64', (8, 3)), 'unit_resistance_median': ('float64', (8, 3)), 'unit_resistance_mode': ('float64', (8, 3)),
    'unit_resistance_credible_range': ('float64', (8, 3)), 'unit_resistance_percentile_5': ('float64', (8, 3)), 'unit_resistance_percentile_50': ('float64', (8,
    3)), 'unit_resistance_percentile_95': ('float64', (8, 3)), 'unit_thickness': ('float64', (8, 3)), 'first_depth_median': ('float64', (8,)),
    'first_depth_percentile_5': ('float64', (8,)), 'first_depth_percentile_50': ('float64', (8,)), 'first_depth_percentile_95': ('float64', (8,)),
    'first_probability': ('float64', (8,)), 'data_exceedance': ('float64', (8, 12)), 'data_outside': ('float64', (8, 12)), 'data_total': ('float64', (8, 12)),
    'data_residual_mean': ('float64', (8, 12)), 'data_residual_median': ('float64', (8, 12)), 'data_residual_mode': ('float64', (8, 12)),
    'data_residual_credible_range': ('float64', (8, 12)), 'data_residual_percentile_5': ('float64', (8, 12)), 'data_residual_percentile_50': ('float64', (8,
    12)), 'data_residual_percentile_95': ('float64', (8, 12)), 'data_predicted_median': ('float64', (8, 12)), 'data_predicted_percentile_5': ('float64', (8,
    12)), 'data_predicted_percentile_50': ('float64', (8, 12)), 'data_predicted_percentile_95': ('float64', (8, 12)), 'misfit_median': ('float64', (8,)),
    'misfit_percentile_5': ('float64', (8,)), 'misfit_percentile_50': ('float64', (8,)), 'misfit_percentile_95': ('float64', (8,)), 'misfit_share_below_one':
    ('float64', (8,)), 'misfit_outside': ('float64', (8,)), 'misfit_total': ('float64', (8,)), 'ensemble_k': ('int32', (8, 32)), 'ensemble_edges': ('float64',
    (8, 32, 30)), 'ensemble_sigma': ('float64', (8, 32, 30)), 'ensemble_misfit': ('float64', (8, 32)), 'ensemble_thin': ('int32', (8,)), 'ensemble_ess':
    ('float64', (8, 440)), 'ensemble_rhat': ('float64', (8, 440)), 'ensemble_tau_iterations': ('float64', (8, 440)), 'ensemble_mcse': ('float64', (8, 440)),
    'ensemble_ess_k': ('float64', (8,)), 'ensemble_ess_misfit': ('float64', (8,)), 'ensemble_rhat_k': ('float64', (8,)), 'ensemble_rhat_misfit': ('float64',
    (8,)), 'ensemble_ess_min': ('float64', (8,)), 'ensemble_resolution_length': ('float64', (8, 440)), 'ensemble_resolution_cells': ('int32', (8, 440)),
    'ensemble_resolution_closed': ('bool', (8, 440)), 'ensemble_correlation_band': ('float64', (8, 440, 5)), 'ensemble_families_n': ('int32', (8,)),
    'ensemble_family_share': ('float64', (8, 2)), 'ensemble_family_silhouette': ('float64', (8, 2)), 'ensemble_family_k': ('int32', (8, 2)),
    'ensemble_family_edges': ('float64', (8, 2, 30)), 'ensemble_family_sigma': ('float64', (8, 2, 30)), 'ensemble_central_k': ('int32', (8,)),
    'ensemble_central_edges': ('float64', (8, 30)), 'ensemble_central_sigma': ('float64', (8, 30)), 'ensemble_central_mean_distance': ('float64', (8,)), 'rhat':
    ('float64', (8, 440)), 'jsd': ('float64', (8, 440)), 'n_used': ('int64', (8, 440)), 'chain_mean': ('float64', (8, 2, 440)), 'rhat_layers': ('float64',
    (8,)), 'jsd_layers': ('float64', (8,)), 'rhat_interfaces': ('float64', (8,)), 'rhat_max': ('float64', (8,)), 'replicates_used': ('int64', (8,)),
    'iterations': ('int64', (8,)), 'acceptance': ('float64', (8,))}

ONE_OF_EACH = {
    'line': ('float64', (8,)), 'fiducial': ('float64', (8,)), 'x': ('float64', (8,)), 'y': ('float64', (8,)), 'z': ('float64', (8,)), 'elevation': ('float64',
    (8,)), 'depth_bin_width': ('float64', ()), 'status': ('int32', (8,)), 'burned_in_iteration': ('int32', (8,)), 'misfit': ('float64', (8,)), 'relative_error':
    ('float64', (8,)), 'additive_error': ('float64', (8,)), 'n_layers': ('int32', (8,)), 'best_n_layers': ('int32', (8,)), 'best_posterior': ('float64', (8,)),
    'best_edges': ('float64', (8, 30)), 'best_conductivity': ('float64', (8, 30)), 'layer_count_posterior': ('int64', (8, 31)), 'interface_posterior': ('int64',
    (8, 440)), 'relative_error_posterior': ('int64', (8, 99)), 'additive_error_posterior': ('int64', (8, 99)), 'mean_log10_conductivity': ('float64', (8, 440)),
    'log10_conductivity_p05': ('float64', (8, 440)), 'log10_conductivity_p50': ('float64', (8, 440)), 'log10_conductivity_p95': ('float64', (8, 440)),
    'ensemble_k': ('int32', (8, 1)), 'ensemble_edges': ('float64', (8, 1, 30)), 'ensemble_sigma': ('float64', (8, 1, 30)), 'ensemble_misfit': ('float64', (8,
    1)), 'ensemble_thin': ('int32', (8,)), 'ensemble_families_n': ('int32', (8,)), 'ensemble_family_share': ('float64', (8, 1)), 'ensemble_family_silhouette':
    ('float64', (8, 1)), 'ensemble_family_k': ('int32', (8, 1)), 'ensemble_family_edges': ('float64', (8, 1, 30)), 'ensemble_family_sigma': ('float64', (8, 1,
    30)), 'ensemble_central_k': ('int32', (8,)), 'ensemble_central_edges': ('float64', (8, 30)), 'ensemble_central_sigma': ('float64', (8, 30)),
    'ensemble_central_mean_distance': ('float64', (8,)), 'iterations': ('int64', (8,)), 'acceptance': ('float64', (8,))}


def _soundings():
    o = survey.read_options(OPTIONS)
    return survey.FdemData.read_csv(o["data_filename"], o["system_filename"]).subset(np.arange(0, 79, 10))      # (as tests/golden/make_device_h5.py)


def _dtypes_and_shapes(res):
    return {k: (np.asarray(v).dtype.name, np.asarray(v).shape) for k, v in res.items()}


def test_every_product_keeps_its_dtype_and_shape():
    res = survey.infer(OPTIONS, data=_soundings(), replicates=2, units={"kind": "depth", "edges": [0.0, 10.0, 30.0, 75.0]}, first_above=(0.1,),
                       data_posteriors=True, ensemble=16, ensemble_diagnostics=dict(max_lag=7), ensemble_correlation=dict(band=4, keep_band=True),
                       ensemble_families=dict(max_families=2), **SHORT)
    assert _dtypes_and_shapes(res) == ALL_PRODUCTS and list(res) == list(ALL_PRODUCTS)


def test_single_columns_keep_their_declared_axis():
    """One kept model of one chain and one family: ``ensemble_k`` [S, 1], ``ensemble_family_share`` [S, 1] keep the axis of width one,
    ``relative_error`` (one error group) comes back [S]."""
    res = survey.infer(OPTIONS, data=_soundings(), ensemble=1, ensemble_families=dict(max_families=1), **SHORT)
    assert _dtypes_and_shapes(res) == ONE_OF_EACH and list(res) == list(ONE_OF_EACH)
    assert res["ensemble_k"].shape == (8, 1) and res["ensemble_family_share"].shape == (8, 1) and res["relative_error"].shape == (8,)
