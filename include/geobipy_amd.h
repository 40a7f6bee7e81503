/*
 * geobipy_amd.h -- C ABI of libgeobipy_amd.so: the MI355X (gfx950) implementation of GeoBIPy's
 * per-sounding hot path (1-D layered-earth FDEM forward solve, its Jacobian, Gaussian data misfit
 * and log-likelihood), batched over soundings.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every function returns gbp_status, 0 = ok.
 *   - pointers marked [dev] are DEVICE pointers (HBM, fp64/int32, C-contiguous); pointers marked
 *     [host] are host pointers.  The library never allocates or frees caller memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Launches are
 *     stream-ordered; the library never synchronises behind the caller's back.
 *   - the acquisition system (filter tables, per-frequency constants) is uploaded once into an
 *     opaque handle; the caller keeps ownership of the arrays passed to gbp_fdem_system_create.
 *
 * Reference interfaces replaced (paths under /root/reference/geobipy/src/classes/):
 *   nbFdem1dfwd            forwardmodelling/Electromagnetic/FD/fdem1d_numba.py:24-68
 *   nbFdem1dsen            forwardmodelling/Electromagnetic/FD/fdem1d_numba.py:71-121
 *   fdem1dfwd / fdem1dsen  forwardmodelling/Electromagnetic/FD/fdem1d.py:10-52, 87-129
 *   DataPoint.std          data/datapoint/DataPoint.py:268-282
 *   EmDataPoint.active     data/datapoint/EmDataPoint.py:44-56
 *   DataPoint.data_misfit  data/datapoint/DataPoint.py:502-525
 *   DataPoint.likelihood   data/datapoint/DataPoint.py:491-500 (-> statistics/MvNormalDistribution.py:201-216)
 */
#ifndef GEOBIPY_AMD_H
#define GEOBIPY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int gbp_status;
enum {
    GBP_OK = 0,
    GBP_ERR_INVALID_ARG = -1,   /* NULL pointer, non-positive size, nF > GBP_MAX_FREQ ...            */
    GBP_ERR_UNSUPPORTED_TID = -2, /* tensor id outside {1, 3, 7, 9}: the reference leaves H undefined
                                     for those (fdem1d_numba.py:57-66); we refuse                     */
    GBP_ERR_BAD_SYSTEM = -3,    /* non-finite / non-positive frequency or separation                  */
    GBP_ERR_HIP = -4,           /* a HIP runtime call failed; see gbp_last_error()                    */
    GBP_ERR_NO_DEVICE = -5      /* no gfx950 device visible                                           */
};

#define GBP_MAX_FREQ 128  /* frequencies per system (TDEM: components x spline nodes) */
#define GBP_NC0 120       /* J0 filter length  (fdem1d_numba.py:18) */
#define GBP_NC1 140       /* J1 filter length  (fdem1d_numba.py:19) */

typedef struct gbp_fdem_system gbp_fdem_system;

/* Library / device info ------------------------------------------------------------------ */
const char *gbp_version(void);
const char *gbp_last_error(void);          /* thread-local text of the last failure            */
gbp_status gbp_device_count(int *count);   /* [host] out                                        */

/*
 * Acquisition system: the per-system arguments of nbFdem1dfwd (fdem1d_numba.py:25), i.e. exactly
 * what FD/fdem1d.py:31-49 extracts from an FdemSystem, all [host], length nF unless noted:
 *   tid          tensor_id = 1 + 3*rx_orient + tx_orient       (system/FdemSystem.py:199-203)
 *   frequencies  Hz
 *   tx_z, rx_z   vertical loop offsets: tHeight = altitude + tx_z, rHeight = -tHeight + rx_z
 *   tx_moment    `moments` argument;  scale = tx_moment * rx_moment
 *   rx_off       loop_offsets[0, :] (x separation), separation = |rx - tx|
 *   w0[120], lamda0[nF,120], w1[140], lamda1[nF,140]  filter weights / abscissae
 *                                                               (system/FdemSystem.py:67-101, 279-337)
 * The handle owns device copies of derived tables; destroy with gbp_fdem_system_destroy.
 */
gbp_status gbp_fdem_system_create(int nF, const int32_t *tid, const double *frequencies,
                                  const double *tx_z, const double *rx_z, const double *tx_moment,
                                  const double *scale, const double *rx_off, const double *separation,
                                  const double *w0, const double *lamda0, const double *w1,
                                  const double *lamda1, gbp_fdem_system **out);
/*
 * Generic Hankel-kernel system from caller-built tables (used by the TDEM path, whose frequency-domain
 * stage is the same layered-earth recursion at quasi-static spline-node frequencies; replaces the
 * frequency-domain part of gatdaem1d's forwardmodel, call site TD/tdem1d.py:89-96).  All [host]:
 *   npts[nF]      abscissa points of each frequency (>= 64)
 *   wmu[nF]       omega * mu0;  hd0[nF]: exponent height offset, hDiff = hd0 - 2 * altitude
 *   g[2 nF]       complex output scale per frequency (re, im)
 *   tables        7 arrays of P = sum(npts) doubles: a = lambda^2 | u0.re | u0.im | coef.re | coef.im |
 *                 ue.re | ue.im   (term = rTE * exp(ue * hDiff) * coef, summed per frequency)
 * The resulting handle is used with gbp_fdem_forward: pred[b] = [Re(out_f), Im(out_f)].
 */
gbp_status gbp_hankel_system_create_raw(int nF, const int32_t *npts, const double *wmu, const double *hd0,
                                        const double *g, const double *tables, gbp_fdem_system **out);
/*
 * Same system with an accuracy-budgeted abscissa window (opt-in): abscissae whose contribution to ANY output
 * is provably (|rTE| <= 1) below eps_ppm in total, for every sounding at altitude >= min_altitude, are left
 * out of the tables (typically half of the 120 at eps_ppm = 1e-12).  eps_ppm <= 0 = all abscissae, i.e.
 * gbp_fdem_system_create.  The Jacobian kernels use the same window (see gbp_fdem_system_create_binned for the bound).
 */
gbp_status gbp_fdem_system_create_windowed(int nF, const int32_t *tid, const double *frequencies,
                                           const double *tx_z, const double *rx_z, const double *tx_moment,
                                           const double *scale, const double *rx_off, const double *separation,
                                           const double *w0, const double *lamda0, const double *w1,
                                           const double *lamda1, double eps_ppm, double min_altitude,
                                           gbp_fdem_system **out);
/*
 * The same window chosen PER SOUNDING: n_bins table sets, set i windowed for altitudes >= first_altitude_m + i metres; the
 * forward kernels look up a sounding's set from its own altitude (below first_altitude_m: all abscissae; above the last bin:
 * the last set, whose bound still holds).  What is evaluated for a sounding therefore depends on that sounding alone --
 * results do not change with the batch a sounding is evaluated in -- and every output stays within eps_ppm of the full
 * 120 / 140-point sums (geobipy_amd's default 1e-10 ppm: two orders below the rounding error of those sums themselves, three
 * below the parity bar).  This is the handle geobipy_amd.FdemBatch and DeviceChains use by default.  The Jacobian kernels and
 * the sampler (gbp_rj_run*) use the same per-sounding sets: rTE is analytic in each layer's conductivity and bounded by 1 on the
 * right half plane, hence |d rTE / d ln sigma_k| <= 2/pi, and the terms dropped from a true-derivative entry obey the same bound.
 */
gbp_status gbp_fdem_system_create_binned(int nF, const int32_t *tid, const double *frequencies,
                                         const double *tx_z, const double *rx_z, const double *tx_moment,
                                         const double *scale, const double *rx_off, const double *separation,
                                         const double *w0, const double *lamda0, const double *w1,
                                         const double *lamda1, double eps_ppm, int first_altitude_m, int n_bins,
                                         gbp_fdem_system **out);
/*
 * Per-sounding windows for ANY handle (gbp_fdem_system_create, gbp_hankel_system_create_raw): builds the n_bins table sets
 * from the handle's own tables, replacing an earlier set.  relative = 0: eps in the units of the output (ppm for gbp_fdem
 * systems; gbp_fdem_system_create_binned = create + this).  relative = 1: eps as a fraction of the value a frequency's sum takes
 * for rTE = 1 at the bin's altitude (the image-source field, the largest the output gets) -- for raw tables whose outputs are not
 * ppm: the time-domain nodal spectra (geobipy_amd.TdemBatch and gbp_tdem_forward use 1e-12).  _clear_bins: back to all abscissae.
 */
gbp_status gbp_hankel_system_add_bins(gbp_fdem_system *sys, double eps, int relative, int first_altitude_m, int n_bins);
gbp_status gbp_hankel_system_clear_bins(gbp_fdem_system *sys);
/*
 * Further table sets for one handle -- the same frequencies, weights and point counts as the tables it was created with, other
 * altitude terms hd0[nF] and points tables[7][P]: e.g. the Hankel tables of other transmitter-receiver offsets of a time-domain
 * system.  The `set_of_row` ARGUMENT of gbp_fdem_forward_rows_ex / gbp_fdem_fm_dlogc_rows_ex (and gbp_td_operator.table_set for
 * the sampler) then makes row b of that launch use set set_of_row[b] (0 = the handle's own tables, k = the k-th added set; [dev]
 * int32, B entries, owned by the caller, read by the kernels; NULL = set 0 for every row), so soundings of different geometry
 * run in ONE launch.  The handle keeps no per-call state: host threads may share one handle, each with its own rows (SURVEY 8b
 * "Threading"; tests/c_abi/two_threads.cpp).  Call gbp_hankel_system_add_bins after the last add_set (eps = 0, n_bins = 0 for "no
 * windows"): it builds every set's descriptors.  Set ids are not range-checked.
 */
gbp_status gbp_hankel_system_add_set(gbp_fdem_system *sys, const double *hd0, const double *tables);
/* abscissa points a sounding at (integer) altitude_m is evaluated with */
gbp_status gbp_fdem_system_bin_points(const gbp_fdem_system *sys, int altitude_m, int *npts);
void gbp_fdem_system_destroy(gbp_fdem_system *sys);
gbp_status gbp_fdem_system_npoints(const gbp_fdem_system *sys, int *npts);  /* abscissa points evaluated per sounding */
gbp_status gbp_fdem_system_nfreq(const gbp_fdem_system *sys, int *nF);
/* free-space field H0 per frequency as (re, im) pairs, [host] out[2*nF] (fdem1d_numba.py:68 denominator) */
gbp_status gbp_fdem_system_h0(const gbp_fdem_system *sys, double *out);

/*
 * Batched forward solve.  Replaces B calls of FdemDataPoint.forward -> fdem1dfwd -> nbFdem1dfwd.
 *   nlayers [dev] int32[B]        layers per sounding (1 <= nlayers[b] <= Lmax); nlayers[b] == 0 skips sounding b:
 *                                 none of its outputs are written (forward, fused and Jacobian entries alike)
 *   sigma   [dev] f64[B, Lmax]    conductivity S/m          (Model.values)
 *   thk     [dev] f64[B, Lmax]    layer thickness m; entry nlayers[b]-1 (the half-space, inf in the
 *                                 reference's mesh.widths) is never read
 *   height  [dev] f64[B]          sensor altitude above the top of the model (DataPoint.z)
 *   pred    [dev] f64[B, 2*nF]    out: [Re(out_0..F-1), Im(out_0..F-1)] in ppm
 *                                 (data/datapoint/FdemDataPoint.py:544-545)
 */
gbp_status gbp_fdem_forward(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                            const double *sigma, const double *thk, const double *height,
                            double *pred, void *stream);

/* Same with an explicit number of waves per workgroup (1..16; 0 = chosen from the batch size, as gbp_fdem_forward does).
 * The partial Hankel sums of a frequency are combined in a fixed order PER wave count, so results are bit-reproducible
 * for a given `waves` and differ in the last digits between wave counts; callers that need results independent of the
 * batch size (sharded surveys) pass the same `waves` everywhere.  There is no hidden per-thread or environment state. */
gbp_status gbp_fdem_forward_ex(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                               const double *sigma, const double *thk, const double *height,
                               double *pred, int waves, void *stream);

/* Same with a table set per row (gbp_hankel_system_add_set): set_of_row [dev] int32[B] or NULL. */
gbp_status gbp_fdem_forward_rows_ex(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                    const double *sigma, const double *thk, const double *height,
                                    double *pred, const int32_t *set_of_row, int waves, void *stream);

/*
 * Per-sounding status word (SURVEY 8b "Errors"; the reference asserts on the host, FD/fdem1d.py:29,
 * DP/FdemDataPoint.py:541, and lets NaNs run): status [dev] int32[B] out, OR of the GBP_ROW_* bits.  `pred` [dev]
 * f64[B, N] may be NULL (inputs only).  The compute entries never abort a batch for one bad row: a row with
 * nlayers[b] > Lmax (or > max_layers of the Jacobian entries) gets NaN outputs and nothing outside its own rows is
 * touched; nlayers[b] <= 0 rows are skipped; non-positive sigma / thickness propagate to NaN / inf in that row only.
 */
enum {
    GBP_ROW_BAD_NLAYERS = 1,       /* nlayers[b] < 1 or > Lmax                                   */
    GBP_ROW_BAD_SIGMA = 2,         /* a used conductivity is not finite and > 0                  */
    GBP_ROW_BAD_THICKNESS = 4,     /* a used thickness (all but the last layer) is not finite and > 0 */
    GBP_ROW_BAD_HEIGHT = 8,        /* altitude negative or not finite (FD/fdem1d.py:29)          */
    GBP_ROW_NONFINITE_OUTPUT = 16  /* a NaN / inf among the sounding's N predicted values        */
};
gbp_status gbp_fdem_validate(int B, int Lmax, int N, const int32_t *nlayers, const double *sigma, const double *thk,
                             const double *height, const double *pred, int32_t *status, void *stream);

/*
 * Gaussian data misfit + log-likelihood for B soundings of N channels each.
 *   pred, obs [dev] f64[B, N];  rel, add [dev] f64[B] (one relative / additive error per sounding,
 *   DataPoint.py:274);  chi2, logL [dev] f64[B] out.
 *   std_i = sqrt((rel*obs_i)^2 + add^2); channel i active iff obs_i > 0 and not NaN;
 *   chi2 = sum_active ((pred-obs)/std)^2;  logL = -(Na/2) ln 2pi - sum_active ln std - chi2/2.
 */
gbp_status gbp_gauss_loglike(int B, int N, const double *pred, const double *obs, const double *rel,
                             const double *add, double *chi2, double *logL, void *stream);

/* Same with an explicit standard deviation per channel, sd [dev] f64[B, N] (TdemDataPoint.std,
 * data/datapoint/TdemDataPoint.py:329-376, is time-gate dependent). */
gbp_status gbp_gauss_loglike_std(int B, int N, const double *pred, const double *obs, const double *sd,
                                 double *chi2, double *logL, void *stream);

/*
 * Fused forward + misfit + log-likelihood (one launch; what Inference1D.accept_reject evaluates at
 * every proposal, inversion/Inference1D.py:572-597).  pred may be NULL when only chi2 / logL are wanted.
 */
gbp_status gbp_fdem_forward_loglike(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                    const double *sigma, const double *thk, const double *height,
                                    const double *obs, const double *rel, const double *add,
                                    double *pred, double *chi2, double *logL, void *stream);

gbp_status gbp_fdem_forward_loglike_ex(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                       const double *sigma, const double *thk, const double *height,
                                       const double *obs, const double *rel, const double *add,
                                       double *pred, double *chi2, double *logL, int waves, void *stream);

/*
 * The same launch with the likelihood's model-independent terms prepared once, for callers that evaluate many models against
 * data and error levels that stay put (proposal rounds over one batch); a single evaluation is cheaper through the plain entry.
 *   gbp_gauss_prepare: obs [dev] f64[B, N], rel, add [dev] f64[B] -> weight [dev] f64[B, N] out (1 / std_i of the active
 *   channels, 0 elsewhere) and c0 [dev] f64[B] out (-(Na/2) ln 2pi - sum_active ln std).  Prepare again whenever obs, rel or add change.
 *   gbp_fdem_forward_loglike_prepared[_ex]: as gbp_fdem_forward_loglike[_ex] with weight, c0 in place of rel, add; chi2, logL and
 *   pred carry the same bits (logL = c0 - chi2/2, every sum in the order of the plain entry).
 */
gbp_status gbp_gauss_prepare(int B, int N, const double *obs, const double *rel, const double *add, double *weight,
                             double *c0, void *stream);

gbp_status gbp_fdem_forward_loglike_prepared(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                             const double *sigma, const double *thk, const double *height,
                                             const double *obs, const double *weight, const double *c0,
                                             double *pred, double *chi2, double *logL, void *stream);

gbp_status gbp_fdem_forward_loglike_prepared_ex(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                                const double *sigma, const double *thk, const double *height,
                                                const double *obs, const double *weight, const double *c0,
                                                double *pred, double *chi2, double *logL, int waves, void *stream);

/*
 * Batched Jacobian d pred / d ln(sigma_k) (ppm).  Replaces FdemDataPoint.sensitivity -> fdem1dsen ->
 * nbFdem1dsen.   J [dev] f64[B, 2*nF, Lmax] out (columns >= nlayers[b] are set to 0);
 * rows [0,nF) real part, [nF,2nF) imaginary part (FdemDataPoint.py:553-557).
 */
gbp_status gbp_fdem_sensitivity(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                const double *sigma, const double *thk, const double *height,
                                double *J, void *stream);

/*
 * Same with two knobs:
 *   max_layers  an upper bound of nlayers[] known to the caller (sizes the kernel's LDS working set;
 *               pass Lmax when unknown).  A sounding with nlayers > max_layers gets a NaN row (J and pred).
 *   exact       0: reproduce the reference's M1_1 formula bit-for-tolerance (default of
 *               gbp_fdem_sensitivity); 1: the true derivative of the forward recursion -- the reference's
 *               expression at fdem1d_numba.py:269-274 is not.
 */
gbp_status gbp_fdem_sensitivity_ex(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                   const double *sigma, const double *thk, const double *height,
                                   double *J, int max_layers, int exact, void *stream);

/*
 * Prediction AND Jacobian of the same models from one pass: FdemDataPoint.fm_dlogc (DP/FdemDataPoint.py:547-551,
 * = forward + sensitivity).  Arguments as gbp_fdem_sensitivity_ex; pred [dev] f64[B, 2*nF] out (may be NULL).
 * Each frequency's Hankel sum is formed by one wave, so `pred` does not depend on the launch shape; it equals
 * gbp_fdem_forward's to rounding (different summation order).
 */
gbp_status gbp_fdem_fm_dlogc(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                             const double *sigma, const double *thk, const double *height,
                             double *pred, double *J, int max_layers, int exact, void *stream);

/* `waves` (0..16): waves per workgroup, a performance hint only -- one wave owns a frequency, so neither J nor pred depend on it. */
gbp_status gbp_fdem_fm_dlogc_ex(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                const double *sigma, const double *thk, const double *height,
                                double *pred, double *J, int max_layers, int exact, int waves, void *stream);

/* Same with a table set per row (gbp_hankel_system_add_set): set_of_row [dev] int32[B] or NULL. */
gbp_status gbp_fdem_fm_dlogc_rows_ex(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                     const double *sigma, const double *thk, const double *height,
                                     double *pred, double *J, int max_layers, int exact, const int32_t *set_of_row,
                                     int waves, void *stream);

/* The two row entries with one more per-row argument (round 4): row_scale [dev] f64[B] or NULL.  Row b is evaluated with the points of
 * its table set taken to the horizontal distance rho_set / row_scale[b] -- abscissae x s, coefficients x s^3 (csrc/gbp_fdem_point.h
 * scale_point): exact for raw Hankel handles of DIPOLE sources (time-domain systems without ModellingLoopRadius), whose tables depend on
 * the distance through lam = base / rho only.  How the time-domain sampler evaluates a SAMPLED receiver position (gbp_td_moves) with the
 * chain's own table set instead of building tables per proposal; a changed dz or transmitter height enters through `height`
 * (2 h + dz = 2 (h + (dz - dz_set) / 2) + dz_set).  NULL: the `_ex` entries. */
gbp_status gbp_fdem_forward_rows_scaled(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                        const double *sigma, const double *thk, const double *height, double *pred,
                                        const int32_t *set_of_row, const double *row_scale, int waves, void *stream);
gbp_status gbp_fdem_fm_dlogc_rows_scaled(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                         const double *sigma, const double *thk, const double *height,
                                         double *pred, double *J, int max_layers, int exact, const int32_t *set_of_row,
                                         const double *row_scale, int waves, void *stream);

/* NOT part of the product interface -- timing helper for bench.py: average kernel time (ms) of `reps` launches of the
 * fused kernel, measured with hipEvents recorded on `stream` around the launches. */
gbp_status gbp_bench_time_forward_loglike(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                         const double *sigma, const double *thk, const double *height,
                                         const double *obs, const double *rel, const double *add,
                                         double *pred, double *chi2, double *logL, void *stream,
                                         int reps, float *avg_ms);

gbp_status gbp_bench_time_forward_loglike_prepared(const gbp_fdem_system *sys, int B, int Lmax, const int32_t *nlayers,
                                                  const double *sigma, const double *thk, const double *height,
                                                  const double *obs, const double *weight, const double *c0,
                                                  double *pred, double *chi2, double *logL, void *stream,
                                                  int reps, float *avg_ms);

/* Test hook: element-wise evaluation of the device math kernels (geobipy_amd/csrc/gbp_math.h) on
 * [dev] arrays of length n.  op: 0 exp_neg(x), 1 sincos(x) -> (sin, cos), 2 csqrt(x + i y) -> (re, im),
 * 3 rcp(x), 4 raw v_rsq_f64 seed, 5 raw v_rcp_f64 seed, 6 sqrt_rsqrt(x) -> (sqrt, 1/sqrt), 7 log_pos(x) (the sampler's ln),
 * 8 sincos_quadrant(x) -> (sin, cos) (the sampler's Box-Muller angle).
 * y and out1 may be NULL where unused. */
gbp_status gbp_debug_math(int op, int n, const double *x, const double *y, double *out0, double *out1,
                          void *stream);

/* ------------------------------------------------------------------------------------------------
 * Device-resident rjMCMC step: one iteration of Inference1D.accept_reject
 * (inversion/Inference1D.py:537-631) for B soundings at once, FDEM data, Resolve-style option set
 * (layer conductivities + relative / additive error; no height move).  Pieces restated per chain:
 *   structural move      RectilinearMesh1D.perturb            mesh/RectilinearMesh1D.py:1018-1118
 *   value remapping      Model.perturb_structure / insert / delete  model/Model.py:316-366
 *   value proposal       Model.stochastic_newton_perturbation model/Model.py:368-419
 *   error proposals      DataPoint.perturb                    data/datapoint/DataPoint.py:531-573
 *   priors               Model.probability :533-575, DataPoint.probability :454-489
 *   jump proposal ratio  Model.proposal_probabilities         model/Model.py:577-659
 *   accept / bookkeeping Inference1D.accept_reject :597-631, update :705-790
 * Same Markov kernel as the reference; the random numbers come from a counter-based generator
 * (Philox4x32-10 keyed by `seed`, counter = chain, iteration, stream, draw), so a chain is a valid
 * draw of the same sampler, not the reference's own draw for a numpy seed (the host-side
 * geobipy_amd.Inference1D does that).  All arrays are [dev]; [B, K] arrays have row stride K.
 */
typedef struct gbp_rj_options {
    int32_t max_layers;          /* K = maximum_number_of_layers                                      */
    int32_t n_channels;          /* N = 2 * nF                                                         */
    int32_t solve_gradient, solve_value;  /* which model priors enter the probability (solve_gradient / solve_parameter) */
    int32_t solve_relative_error, solve_additive_error, exact_jacobian;
    int32_t n_depth_bins, n_value_bins;   /* posterior grids (interface histogram / hit-map)          */
    int32_t n_error_bins;        /* cells of the error-level histograms (log10 between the prior bounds; reference: 99) */
    int32_t schedule;            /* 0: the caller decides what is accumulated (`accumulate` argument);
                                    1: the reference's per-sounding schedule (Inference1D.update :713-737, infer :641-688):
                                       a chain burns in at the first iteration > burn_in_min_iterations with misfit <
                                       active channels -- its posteriors and best model start over there --, is done
                                       n_markov_chains iterations later, and has failed when it has not burned in after
                                       n_markov_chains iterations; done / failed chains keep their final state          */
    int32_t burn_in_min_iterations, n_markov_chains;
    int32_t forward_waves;       /* waves per sounding of the forward launches (and per chain of the persistent kernel):
                                    0 = chosen from the block size, > 0 = fixed.  A performance hint only: the Hankel sums
                                    are reduced per 64-point pass and added in pass order, so the chains are bit-identical
                                    for any value, block size and sharding of the survey                 */
    double min_edge, max_edge, min_width; /* min_edge already raised to min_width (RectilinearMesh1D.py:358-360) */
    double p_birth, p_death, p_perturb, p_none;
    double value_precision;      /* 1 / ln(1 + factor)^2                                              */
    double value_min, value_max; /* parameter_limits: proposals with a conductivity outside have zero prior; value_max <= 0: none */
    double gradient_precision;   /* 1 / gradient_standard_deviation^2                                 */
    double alpha;                /* covariance_scaling                                                 */
    int32_t n_rel_groups, n_add_groups;   /* error levels per sounding, 1..4 each: one relative level per system x component and
                                             one additive level per system (DataPoint.py:268-282, TdemDataPoint.py:361-365);
                                             frequency-domain data with one system: 1 and 1                              */
    double rel_min[4], rel_max[4], rel_sd[4], add_min[4], add_max[4], add_sd[4];   /* per group; sd = sqrt(proposal variance) */
    double depth_bin_width;      /* interface histogram / hit-map depth cell                           */
    double value_half_width;     /* hit-map spans log10(sigma / prior mean) in [-w, w]                 */
    uint64_t seed;
    uint64_t first_chain;        /* global index of chain 0 of this block: the random streams are keyed by
                                    first_chain + b, so a survey gives the same chains however it is sharded */
    /* The height move of the data point (`solve_z`: Point.perturb / set_priors / set_proposals, pointcloud/Point.py:614-621,
     * 949-983): uniform prior height0 +- height_half_width (maximum_z_change), random walk height + height_scale * N(0, 1)
     * redrawn up to 10 times while outside the prior, then kept.  height_scale is the reference's `z_proposal_variance` AS IS:
     * its NormalDistribution.rng passes the variance to numpy as the scale (statistics/NormalDistribution.py:111).  Needs
     * chains->height_p and ->height0; chains->height is then STATE (written on acceptance).  Lock-step drivers only. */
    int32_t solve_height;
    double height_half_width, height_scale;
    int32_t additive_independent;/* the additive levels as Tempest_datapoint treats its additive-error MULTIPLIERS (data/datapoint/
                                    Tempest_datapoint.py:339-341, 475-487, 503-508): ONE joint draw per iteration from a log-normal
                                    centred on add_centre (where set_proposals put it: the initial multipliers -- the proposal's mean
                                    is never moved to the state, so this is an independence sampler, not a random walk), no redraw
                                    against the prior, and no prior term in the acceptance ratio.  0: the levels of every other data
                                    point (random walk, redrawn while outside the log-uniform prior, prior in the ratio)          */
    double add_centre[4];
    double extra_log_prior;      /* constant added to every proposal's log prior: the densities of the uniform priors of sampled
                                    scalars that live outside the chains struct, in gbp_td_moves; cancels in the acceptance ratio, keeps
                                    the stored prior / posterior values those of the full model                              */
    int32_t trace_every, trace_length; /* per-iteration traces (chains->trace_misfit / trace_accept; Inference1D.data_misfit_v / acceptance_v,
                                    inversion/Inference1D.py:408, 414, 713, 749): every `trace_every`-th entry of the reference's two
                                    arrays is kept, `trace_length` slots per chain -- slot j holds data_misfit_v[j * trace_every] (the misfit
                                    after update j * trace_every + 1) and acceptance_v[j * trace_every] (the decision of update j *
                                    trace_every), updates counted from the chain's (re)start.  trace_every = 1, trace_length = 2 *
                                    n_markov_chains: the reference's arrays in full.  0: no traces                                  */
    /* Sampled unit posteriors (chains->unit_z ...): properties of a depth unit [z0, z1] of every SAMPLED model, binned where the hit
     * map is settled and with the same dwell weight.  Layer l spans [top_l, bot_l), top_0 = 0, bot_{k-1} = +inf; its overlap with the
     * unit is ov_l = max(0, min(bot_l, z1) - max(top_l, z0)); layers with ov_l = 0 are skipped, l ascending, one rounded multiply /
     * divide and one rounded add per term (no fused multiply-add):
     *   arithmetic mean  a = (sum_l sigma_l ov_l) / dz   (conductance over thickness)
     *   harmonic mean    h = dz / (sum_l ov_l / sigma_l) (thickness over transverse resistance)
     * each binned on the hit map's value axis of its chain.  Depth to a threshold: top_l of the shallowest layer with sigma_l >= t
     * (direction +1) or sigma_l <= t (-1), binned on the depth axis as edge_hist bins an interface; no such layer: first_none. */
    int32_t n_units;             /* M, 0 .. 16 units per chain; 0: off                                                    */
    int32_t unit_kinds;          /* bit 0 arithmetic, bit 1 harmonic (1 .. 3 when n_units > 0)                            */
    int32_t n_first;             /* 0 .. 4 thresholds                                                                     */
    double first_threshold[4];   /* S/m, finite and positive                                                              */
    int32_t first_direction[4];  /* +1: first layer at or above the threshold, -1: at or below                            */
    /* Data-space posteriors (chains->data_hist, misfit_hist): the prediction and the misfit of every SAMPLED model, binned where the
     * hit map is settled and with the same dwell weight (a chain's prediction and misfit change only when a proposal is accepted).
     * Channel n of chain b, active when obs = data[b, n] > 0 (inactive channels get no counts), every operation rounded once, in
     * this order (no fused multiply-add):
     *   r   = (pred[n] - obs) / data_scale[b, n]              the residual in scale units
     *   pos = (r + H) / (2 H) * n_data_bins                   H = data_half_width
     *   data_hist[b, clamp(floor(pos), 0, n_data_bins - 1), n] += dwell      (a non-finite pos goes to no cell)
     * and once per chain, with H = misfit_half_width decades:
     *   v   = ln(misfit / misfit_scale[b]) * 0.43429448190325182765          (the sampler's own ln; misfit = chi^2)
     *   pos = (v + H) / (2 H) * n_data_bins
     *   misfit_hist[b, clamp(floor(pos), 0, n_data_bins - 1)] += dwell
     * The end cells hold everything beyond +-H.  The entry points refuse n_data_bins outside 8 .. 256, a half width that is not
     * positive and finite, histograms without hitmap (they share hit_dwell and are zeroed where it is), a histogram without its
     * scale or without the other histogram.  A block that samples the prior alone has no active channel: its data_hist stays 0. */
    int32_t n_data_bins;         /* 0: off; otherwise 8 .. 256 cells of both axes                                        */
    double data_half_width;      /* > 0 and finite: the residual axis spans +-data_half_width scale units                */
    double misfit_half_width;    /* > 0 and finite: the misfit axis spans +-misfit_half_width decades about misfit_scale */
    /* Posterior ensemble (chains->ens_k ...): the SAMPLED MODELS themselves, thinned, kept per chain in chain order.  The samples a
     * chain accumulates are numbered from 0 where its posteriors last started (ens_seen counts them).  A settle of model m with weight
     * d (its dwell: where the hit map is settled, with the same weight) covers the samples n = ens_seen .. ens_seen + d - 1.  Sample n
     * is kept iff n % ensemble_thin == 0 and n / ensemble_thin < n_ensemble, and goes to slot n / ensemble_thin.  One settle therefore
     * writes m into the slots ceil(ens_seen / thin) .. min(n_ensemble - 1, floor((ens_seen + d - 1) / thin)); then ens_seen += d.
     * Samples past the last slot are dropped: no ring, no replacement.  After gbp_rj_flush_posteriors ens_seen equals the sum of
     * k_hist, and min(n_ensemble, ceil(ens_seen / thin)) slots are filled.  The burn-in reset zeroes ens_k and ens_seen.  The entry
     * points refuse n_ensemble outside 1 .. 4096, ensemble_thin < 1, the arrays without hitmap (they share hit_dwell), and one
     * array without the others. */
    int32_t n_ensemble;          /* 0: off; otherwise 1 .. 4096 slots per chain                                          */
    int32_t ensemble_thin;       /* >= 1: every ensemble_thin-th sample is kept                                          */
} gbp_rj_options;

typedef struct gbp_rj_chains {
    int32_t B;
    /* constants */
    const int32_t *rel_group, *add_group;   /* [N] or NULL  group of each channel's relative / additive level; NULL = 0 */
    const double *add_scale;       /* [N] or NULL  per-channel factor of the additive error: std^2 = (rel d)^2 + (add * add_scale)^2
                                      (TdemDataPoint.std, data/datapoint/TdemDataPoint.py:361-365: sqrt(1e-3 / t)); NULL = 1 (FDEM) */
    const int64_t *chain_id;       /* [B] or NULL  global index of each chain (keys its random streams); NULL: first_chain + b */
    const double *data;            /* [B, N]  observed data (<= 0: inactive channel)                   */
    const double *height;          /* [B]     sensor height; with opt->solve_height the chain's CURRENT height: state, written by the
                                      sampler on acceptance (the const is dropped there)                 */
    const double *log_mean_prior;  /* [B]     ln of the best half-space conductivity                   */
    /* chain state */
    int32_t *k;                    /* [B]     layers                                                   */
    double *edges, *sigma;         /* [B, K]  interface depths (k - 1 used, +inf padded), conductivities (1 padded) */
    double *rel, *add;             /* [B, n_rel_groups], [B, n_add_groups]  error levels                                  */
    double *pred, *J;              /* [B, N], [B, N, K]  carried prediction / Jacobian                  */
    double *prior, *like, *misfit; /* [B]                                                              */
    /* proposal scratch (written by the step) */
    int32_t *action, *k_r;         /* [B]     0 none, 1 insert, 2 delete, 3 perturb; layers after the move */
    int32_t *nl_a, *nl_c;          /* [3, B]  k_r of the chains needing the phase A / C kernels, else 0: row 0 all,
                                      rows 1-2 split by layer count (<= 8, more)                         */
    int32_t *nl_b;                 /* [B]     k_r of the chains whose proposal keeps its dimension (fused forward), else 0 */
    double *edges_r, *sigma_r, *thk_r;        /* [B, K] remapped model                                 */
    double *rel_p, *add_p;                    /* [B, n_*_groups]  proposed error levels              */
    double *pred_r, *J_r;                     /* [B, N], [B, N, K] at the remapped model               */
    double *chol;                             /* [B, K, K] lower Cholesky factor of the proposal precision */
    double *log_prop, *sigma_p;               /* [B, K] proposed ln sigma, sigma                       */
    double *pred_p, *misfit_p, *like_p, *J_p; /* proposal: [B, N], [B], [B], [B, N, K]                  */
    double *log_ratio;                        /* [B]   ln acceptance ratio of the last step            */
    /* bookkeeping */
    int64_t *n_accepted;           /* [B]                                                              */
    int32_t *k_hist;               /* [B, K + 1]            posterior of the layer count               */
    int32_t *edge_hist;            /* [B, n_depth_bins]     interfaces with a conductivity contrast > 50 % */
    int32_t *rel_hist, *add_hist;  /* [B, n_*_groups, n_error_bins]  posteriors of the error levels (both or neither; may be NULL) */
    int32_t *hitmap;               /* [B, n_value_bins, n_depth_bins] or NULL (depth fastest: the cells of one layer share a
                                      value bin, so one iteration updates a few contiguous runs)         */
    int32_t *hit_dwell;            /* [B] (with hitmap)  iterations the current model is still owed to the hit map: a model is
                                      added with its dwell time when it is replaced; gbp_rj_flush_posteriors settles the rest */
    int32_t *burned_in_iteration;  /* [B]  schedule 1: -1 until the chain burns in (may be NULL for schedule 0)          */
    int32_t *status;               /* [B]  schedule 1: 0 running, 1 done, 2 failed to burn in                            */
    double *best_posterior;        /* [B]                                                              */
    int32_t *best_k;
    double *best_edges, *best_sigma;          /* [B, K]                                                */
    double *best_rel, *best_add;   /* [B, n_rel_groups], [B, n_add_groups] or NULL: error levels of the highest-posterior state */
    int32_t *iteration0;           /* [B] or NULL (= 0)  schedule 1: the iteration at which the chain (re)started -- the schedule
                                      counts from there (Inference1D.reset :984-999 restarts a chain that accepted nothing over a
                                      whole window; the host does the restart between calls, rjmcmc_gpu.DeviceChains.infer) */
    /* height move (opt->solve_height; all NULL otherwise) */
    double *height_p;              /* [B]  proposed height (scratch of the step)                                          */
    const double *height0;         /* [B]  centre of the uniform prior = the sounding's measured height                   */
    int32_t *height_hist;          /* [B, n_error_bins] or NULL  posterior of the height on the prior's cells (Point.set_z_posterior) */
    double *best_height;           /* [B] or NULL  height of the highest-posterior state                                  */
    int32_t *step_flags;           /* [B] or NULL  what the accept stage did with the chain in the last iteration: bit 0 accepted,
                                      bit 1 the highest-posterior state was replaced, bit 2 the posteriors were reset (burn-in),
                                      bit 3 the post-step state was added to the posteriors; 0 for a frozen chain.  Read by the
                                      stages that carry further per-chain state (gbp_td_moves)                             */
    double *trace_misfit;          /* [B, trace_length] or NULL  decimated misfit trace (opt->trace_every; NaN = not reached)      */
    uint8_t *trace_accept;         /* [B, trace_length] or NULL  decimated accept / reject decisions (both traces or neither)      */
    int32_t *best_iteration;       /* [B] or NULL  the update (1-based, from the chain's (re)start) that produced the highest-posterior
                                      state (Inference1D.best_iteration :733, 743)                                                */
    /* sampled unit posteriors (opt->n_units / n_first; need hitmap: they share hit_dwell and are zeroed where it is; all NULL: off) */
    const double *unit_z;          /* [B, n_units, 2]  top and bottom of every unit, metres below the surface, 0 <= z0 <= z1 finite;
                                      z1 == z0: the unit has no posterior (its column stays 0)                              */
    int32_t *unit_hist;            /* [B, Q, n_value_bins, n_units]  Q = set bits of unit_kinds, arithmetic first; unit fastest:
                                      the layout of the interval marginals (gbp_hitmap_intervals), int32                    */
    int32_t *first_hist;           /* [B, n_first, n_depth_bins]  depth to the first layer beyond each threshold            */
    int32_t *first_none;           /* [B, n_first]  samples without such a layer                                            */
    /* data-space posteriors (opt->n_data_bins; need hitmap: they share hit_dwell and are zeroed where it is; all NULL: off) */
    const double *data_scale;      /* [B, N]  unit of the residual axis of every channel, > 0 and finite on active channels (the
                                      channel's standard deviation at the chain's initial error levels, say)                */
    int32_t *data_hist;            /* [B, n_data_bins, N]  residuals of the sampled predictions; channel fastest: the value-major
                                      layout of the interval marginals, int32                                               */
    const double *misfit_scale;    /* [B]  > 0: what the misfit is divided by (the chain's number of active channels)       */
    int32_t *misfit_hist;          /* [B, n_data_bins]  log10(misfit / misfit_scale) of the sampled models                  */
    /* posterior ensemble (opt->n_ensemble, ensemble_thin; needs hitmap: it shares hit_dwell and is zeroed where it is; all NULL: off) */
    int32_t *ens_k;                /* [B, n_ensemble]  layer count of the slot's model; 0: the slot is empty                */
    double *ens_edges;             /* [B, n_ensemble, K]  the k - 1 interface depths of the slot's model, then +inf         */
    double *ens_sigma;             /* [B, n_ensemble, K]  its k conductivities, then NaN                                    */
    double *ens_misfit;            /* [B, n_ensemble]  its misfit (chi^2: what the data-space posteriors bin at the same site) */
    int32_t *ens_seen;             /* [B]  accumulated samples already settled since the posteriors last started            */
} gbp_rj_chains;

/* The three host-logic stages of one iteration, exposed separately for the tests ... */
gbp_status gbp_rj_propose(const gbp_rj_options *opt, const gbp_rj_chains *c, int64_t iteration, void *stream);
gbp_status gbp_rj_newton(const gbp_rj_options *opt, const gbp_rj_chains *c, int64_t iteration, void *stream);
gbp_status gbp_rj_accept(const gbp_rj_options *opt, const gbp_rj_chains *c, int64_t iteration, int accumulate,
                         void *stream);
/* ... and n_iterations complete iterations (propose, prediction + Jacobian of the remapped models, newton, fused
 * forward + likelihood of the proposals that keep their dimension, prediction + Jacobian of those that change it, accept), all stream-ordered, no host
 * synchronisation.  `accumulate` != 0 adds every post-step state to the posterior histograms. */
gbp_status gbp_rj_run(const gbp_fdem_system *sys, const gbp_rj_options *opt, const gbp_rj_chains *c,
                      int64_t first_iteration, int n_iterations, int accumulate, void *stream);
/* `mode`: 0 = gbp_rj_run's choice, 1 = lock-step driver (stream-ordered launches per iteration over the whole block: propose,
 * the evaluations at the remapped models, Newton (one launch), the evaluations at the proposals, accept (one launch)),
 * 2 = persistent kernel (one workgroup owns a chain and loops over all n_iterations in ONE launch; frequency-domain data),
 * 3 = lock-step with one launch per kind of evaluation and layer-count bucket (ten per iteration; what time-domain blocks use),
 * 4 = lock-step as 1, the block cut into 3 contiguous sub-blocks that advance concurrently on streams of their own (a host thread
 * each for the duration of the call) -- the latency-bound per-chain stages of one overlap the physics of the others: +9 % at 2 048
 * chains, +20 % at 4 096, +25 % at 8 192, +12 % at 16 384.
 * All drivers walk bit-identical chains; small blocks (config 5 split over 8 GPUs: 1 024 chains per GPU) are about twice as
 * fast in mode 2, medium ones (2 048 ... ~20 000 chains) fastest in mode 4 (from about four iterations per call: the sub-blocks'
 * host threads and stream joins are per call), large ones in mode 1.  Mode 0 chooses.  In mode 4 the
 * launch masks nl_a / nl_c hold one [3, n] block per sub-block instead of one [3, B] array (scratch of an iteration). */
gbp_status gbp_rj_run_mode(const gbp_fdem_system *sys, const gbp_rj_options *opt, const gbp_rj_chains *c,
                           int64_t first_iteration, int n_iterations, int accumulate, int mode, void *stream);
/*
 * The same for time-domain data (TdemDataPoint): `sys` is the frequency-domain handle of the spline nodes of the system --
 * or of all systems of a multi-moment acquisition merged into one (gbp_hankel_system_create_raw) --, and a constant block
 * matrix turns the nodal spectrum into window values, windows = nodal @ W (geobipy_amd/tdem.py; replaces gatdaem1d's
 * forwardmodel / derivative, TD/tdem1d.py:89-154).  opt->n_channels = the number of windows; chains->add_scale carries the
 * time-dependent additive error, rel_group / add_group the level of each channel.
 */
/* Geometry mixing (transmitter / receiver attitude, azimuth of the receiver offset, X / Y / Z outputs; geobipy_amd/tdem_geometry.py):
 * the frequency-domain kernels then produce the nodal spectra of the BASIS INTEGRALS of the transmitter-receiver frame
 * (n_in values per row) and the spectrum entry m of the output components is the per-row real combination
 *     out[m] = sum_{t < terms} weights[b, col[m, t]] * in[src[m, t]]        (src < 0: no term)
 * formed inside gbp_td_apply_mix / the sampler's window stage.  n_in = 0: no mixing (the kernels' spectra are the outputs'). */
typedef struct gbp_td_mix {
    int32_t n_in;           /* nodal values per row written by the kernels = 2 * nF of `sys`; 0 = no mixing   */
    int32_t terms;          /* T                                                                              */
    int32_t n_weights;      /* weights per row                                                                */
    const int32_t *src;     /* [dev] int32[n_nodal, T]                                                        */
    const int32_t *col;     /* [dev] int32[n_nodal, T]                                                        */
    const double *weights;  /* [dev] f64[B, n_weights]                                                        */
    const double *offset;   /* [dev] f64[B, n_channels] or NULL: added to the windows of every row -- the predicted PRIMARY
                               field of data whose channels hold primary + secondary (Tempest_datapoint.py:106-123);
                               honoured with or without mixing (n_in = 0)                                      */
} gbp_td_mix;
/* Sampled attitude angles of the loop pair (the reference's solve_transmitter_pitch / _roll / _yaw and solve_receiver_pitch / _roll /
 * _yaw: Loop_pair.perturb system/Loop_pair.py:161-164, EmLoop.perturb / set_priors / set_proposals system/EmLoop.py:222-305 -- the
 * receiver pitch is the nuisance parameter of Tempest inversions).  A rotation changes neither the Hankel tables (they depend on the
 * horizontal distance and dz) nor the kernels' nodal spectra of the basis integrals, only the per-row real mixing weights (and the
 * primary field of total-field data): every chain carries its GA-AEM tuple, a proposal stage draws the angles -- uniform prior
 * centre +- half_width, random walk redrawn up to 10 times while outside, scale = the reference's proposal "variance" as is (see
 * solve_height) -- and forms the proposal's weights / offset; evaluations at proposals use those; the accept stage's decision
 * (chains->step_flags) moves them into the state.  Needs mix.n_in > 0 and chains->step_flags.  n_moves = 0: fixed geometry. */
typedef struct gbp_td_moves {
    int32_t n_moves;             /* 0 .. 6                                                                              */
    int32_t entry[6];            /* entry of the GA-AEM tuple a move samples: 1..3 transmitter roll, pitch, yaw; 7..9 receiver;
                                    with `rho_scale` (position moves): 0 transmitter height, 4..6 receiver offset dx, dy, dz           */
    double sign[6];              /* tuple entry = sign * sampled value (Loop_pair.Geometry negates pitch and yaw)        */
    double half_width[6];        /* maximum_<..>_change                                                                  */
    double scale[6];             /* <..>_proposal_variance, used as the standard deviation like the reference does       */
    int32_t n_bins[6];           /* cells of the posterior on the prior's support: 199 for a pitch, 99 otherwise (<= 199) */
    double *geom, *geom_p;       /* [dev] f64[B, 10] GA-AEM tuples: current (state) and proposed (scratch)                */
    const double *geom0;         /* [dev] f64[B, 10] the measured geometry: prior centres                                */
    double *weights;             /* [dev] f64[B, mix.n_weights] = mix.weights, writable (state)                          */
    double *weights_p;           /* [dev] f64[B, mix.n_weights] (scratch)                                                */
    double *offset, *offset_p;   /* [dev] f64[B, n_channels] = mix.offset writable / its proposal; both NULL without total-field data */
    int32_t *hist;               /* [dev] int32[B, n_moves, 199] or NULL: posteriors                                     */
    double *best_geom;           /* [dev] f64[B, 10] or NULL: tuple of the highest-posterior state                       */
    /* how weights and offset follow from a tuple (geobipy_amd/tdem_geometry.py GeometryMix): one block of n_basis weights per
     * (system, output component) */
    int32_t n_blocks, n_basis, loop, on_axis;
    int32_t basis[5];            /* the basis integrals of the layout, indices into (B0L, B1L, B0, B1, BA)               */
    const int32_t *block_comp;   /* [dev] int32[n_blocks]  0 x, 1 y, 2 z                                                  */
    const double *block_scale;   /* [dev] f64[n_blocks]    output sign * output scaling                                   */
    const double *block_primary; /* [dev] f64[n_blocks]    factor of the free-space field in output units (with offset)   */
    const int32_t *block_windows;/* [dev] int32[n_blocks]  windows of the block (with offset)                             */
    /* Position moves (the reference's solve_receiver_x / _y / _z = the pair's offset, solve_transmitter_z; Loop_pair.perturb :161-164,
     * Point.perturb): a moved receiver keeps its chain's TABLE SET -- built for the measured (rho_set, dz_set) -- and is evaluated with
     * the per-chain scalars  rho_scale = rho_set / rho  (gbp_fdem_*_rows_scaled; dipole sources only when dx / dy move) and the effective
     * height  h + (dz - dz_set) / 2  written to chains->height_p (proposal) / chains->height (state; the const is dropped).  All NULL:
     * angles only.  Needs chains->height_p. */
    double *rho_scale, *rho_scale_p;  /* [dev] f64[B] rho_set / rho of the state / of the proposal (scratch)              */
    const double *rho_set, *dz_set;  /* [dev] f64[B] horizontal distance and dz the chain's table set was built for       */
} gbp_td_moves;
typedef struct gbp_td_operator {
    int32_t n_nodal;        /* rows of W (= 2 * nF of `sys` without mixing)                                   */
    const double *W;        /* [dev] f64[n_nodal, n_channels], row-major                                      */
    double *nodal;          /* [dev] scratch f64[B, max(n_nodal, mix.n_in)]                                   */
    double *J_nodal;        /* [dev] scratch f64[B, max(n_nodal, mix.n_in), K]                                */
    gbp_td_mix mix;         /* geometry mixing, or n_in = 0                                                   */
    const int32_t *table_set;  /* [dev] int32[B] or NULL: table set of every chain (gbp_hankel_system_add_set)  */
    gbp_td_moves moves;     /* sampled attitude angles, or n_moves = 0                                        */
} gbp_td_operator;
/* The time-domain stage on its own (what TdemDataPoint.forward / sensitivity add to the frequency-domain kernels): for every
 * sounding with nlayers[b] > 0,  pred[b, :] = nodal[b, :] @ W  and, when J_nodal / J are given,
 * J[b, g, l] = sum_m J_nodal[b, m, l] W[m, g] for l < nlayers[b] (0 beyond).  All [dev]; nodal f64[B, n_nodal] as written by
 * gbp_fdem_forward on the raw Hankel handle, J_nodal f64[B, n_nodal, K] by gbp_fdem_sensitivity_ex, W f64[n_nodal, N],
 * pred f64[B, N], J f64[B, N, K]. */
gbp_status gbp_td_apply(int B, int K, int n_nodal, int N, const int32_t *nlayers, const double *W, const double *nodal,
                        const double *J_nodal, double *pred, double *J, void *stream);
/* Same with geometry mixing: nodal f64[B, mix->n_in], J_nodal f64[B, mix->n_in, K] (mix NULL or n_in = 0: as gbp_td_apply). */
gbp_status gbp_td_apply_mix(int B, int K, int n_nodal, int N, const int32_t *nlayers, const double *W, const double *nodal,
                            const double *J_nodal, double *pred, double *J, const gbp_td_mix *mix, void *stream);
gbp_status gbp_rj_run_td(const gbp_fdem_system *sys, const gbp_td_operator *td, const gbp_rj_options *opt,
                         const gbp_rj_chains *c, int64_t first_iteration, int n_iterations, int accumulate, void *stream);
/* Adds what the chains' current models are still owed to the hit maps (see hit_dwell); call before reading them. */
gbp_status gbp_rj_flush_posteriors(const gbp_rj_options *opt, const gbp_rj_chains *c, void *stream);
/* ------------------------------------------------------------------------------------------------
 * Time-domain systems at the C level (SURVEY 8b "TDEM boundary"): what the reference gets from GA-AEM's
 *   gatdaem1d.TDAEMSystem(stmfile)                     system/TdemSystem_GAAEM.py:8-35
 *   .forwardmodel(Geometry, Earth) -> SX / SZ          forwardmodelling/Electromagnetic/TD/tdem1d.py:89-96
 *   Geometry(tx_height, tx_roll, -tx_pitch, -tx_yaw, txrx_dx, txrx_dy, txrx_dz, rx_roll, -rx_pitch, -rx_yaw)   system/Loop_pair.py:70-77
 * gbp_tdem_system_create parses the TEXT of a .stm file ([host], NUL-terminated) and folds waveform, spline, low-pass
 * filters and windows into one matrix (geobipy_amd/csrc/gbp_tdem.h); w0[120] / w1[140]: the J0 / J1 Hankel filter weights
 * (the same [host] arrays gbp_fdem_system_create takes).
 * gbp_tdem_forward: geometry [host] f64[B, 10] = GA-AEM's tuple above, angles in degrees in GA-AEM's convention (x = flight
 * direction, y = left, z = up; roll "left side up", pitch "nose down", yaw "turn left" positive; body -> earth matrix
 * Rz(yaw) Ry(pitch) Rx(roll)) -- the reference's sign changes of pitch and yaw are the caller's, as they are in Loop_pair.py.
 * Any attitude and any receiver offset per row, all rows in one launch: the handle keeps one table set per (horizontal
 * distance, dz) it has seen (at most 4096 per layout: bin measured offsets, e.g. to 0.1 m) and a row's azimuth and attitude
 * enter as a per-row mixing matrix of the nodal spectra (gbp_td_mix; geobipy_amd/tdem_geometry.py).  The conventions are restated
 * from GA-AEM's published description and held against closed forms (tests/test_tdem_attitude.py), not against gatdaem1d:
 * parity unpinned for non-zero angles.  nlayers / sigma / thk [dev] as in gbp_fdem_forward; out [dev] f64[B, n_components *
 * n_windows], components x, y, z (those with a non-zero output scaling), in the reference's sign convention for
 * predicted_secondary_field (TdemDataPoint.py:1004-1015).
 * gbp_tdem_fm_dlogc: the same plus J [dev] f64[B, n_components * n_windows, Lmax] = d out / d ln sigma (columns >= nlayers[b]
 * are 0) -- what the reference gets from gatdaem1d's fm_dlogc / derivative(CONDUCTIVITYDERIVATIVE, layer) x sigma
 * (TD/tdem1d.py:98-154), here the exact derivative through the same kernels.
 * Stream-ordered and RE-ENTRANT (SURVEY 8b "Threading"; round 4): host threads may share one handle, each calling on a stream of its
 * own.  A call leases its staging vectors and device scratch from a pool in the handle (the workspace it used last on the same stream,
 * else one whose last call has completed, else a new one); the table sets the calls share are looked up -- and, for a geometry the
 * handle has not met, grown: the device tables are re-allocated then, which waits for the launches that still read the old ones --
 * under the handle's lock, together with the enqueue of the call's launches, so the GPU work of concurrent callers overlaps and only
 * their host-side enqueue takes turns.  Results do not depend on what else the handle has seen or is doing
 * (tests/c_abi/two_threads_tdem.cpp: bit-equal to a fresh handle's single-threaded results while another thread grows the table sets).
 * (The geometry rows and per-sounding heights are HOST arrays read during the call; gbp_tdem_system_set_hankel_eps takes the same lock.)
 */
typedef struct gbp_tdem_system gbp_tdem_system;
gbp_status gbp_tdem_system_create(const char *stm_text, const double *w0, const double *w1, gbp_tdem_system **out);
void gbp_tdem_system_destroy(gbp_tdem_system *sys);
gbp_status gbp_tdem_system_info(const gbp_tdem_system *sys, int *n_windows, int *n_components, int *n_nodes, double *loop_radius);
/* accuracy budget of the per-sounding abscissa windows of gbp_tdem_forward, relative to the inductive-limit value of every nodal
 * sum (default 1e-12: about half of the 120 / 140 abscissae at survey altitudes, far below anything the windows resolve); 0 = all */
gbp_status gbp_tdem_system_set_hankel_eps(gbp_tdem_system *sys, double eps);
/* [host] out: window centres [n_windows] (= gatdaem1d windows.centre), spline-node frequencies [n_nodes], the per-component
 * operator W [2 * n_nodes, n_windows]; any may be NULL */
gbp_status gbp_tdem_system_tables(const gbp_tdem_system *sys, double *window_centres, double *node_frequencies, double *W);
gbp_status gbp_tdem_forward(gbp_tdem_system *sys, int B, const double *geometry, int Lmax, const int32_t *nlayers,
                            const double *sigma, const double *thk, double *out, void *stream);
gbp_status gbp_tdem_fm_dlogc(gbp_tdem_system *sys, int B, const double *geometry, int Lmax, const int32_t *nlayers,
                             const double *sigma, const double *thk, double *out, double *J, void *stream);

/* Diagnostics: [host] out[8] = accumulated 100 MHz clock ticks of chain 0 in the persistent kernel's stages (propose, fm_dlogc at
 * the remapped model, newton, forward / fm_dlogc at the proposal, accept), out[5] = iterations counted, out[6] / out[7] = the longest /
 * the mean life of the launches' workgroups in ticks (a persistent launch ends with its slowest chain); synchronises the device.
 * reset: 0 read only, 1 zero the counters and arm the clock (off by default: it costs chain 0 a few global updates per iteration),
 * 2 zero and disarm. */
gbp_status gbp_rj_debug_stage_ticks(int64_t *out, int reset);
/* Test hook: the proposal stage through one of its three independent implementations of the same draws (0 = gbp_rj_propose's:
 * thread per chain, rows staged through LDS; 1 = unstaged thread per chain; 2 = one wave per chain); an explicit argument, no
 * environment variable or other hidden state. */
gbp_status gbp_rj_debug_propose_variant(const gbp_rj_options *opt, const gbp_rj_chains *c, int64_t iteration, int variant, void *stream);
/* Test hook: n uniforms and n standard normals of stream (chain, iteration, stream_id) as the kernels draw them. */
gbp_status gbp_rj_debug_random(uint64_t seed, int64_t chain, int64_t iteration, int stream_id, int n,
                               double *uniforms, double *normals, void *stream);

/* What leaves the device of a block's conductivity-depth hit maps (int32 [B, n_value, n_depth], depth fastest; csrc/gbp_hitmap.h; the
 * reference derives the same on the host from its Histogram2D posterior, classes/statistics/Histogram.py mean / percentile):
 * gbp_hitmap_statistics -- per depth cell the mean and the 5 / 50 / 95 % points of log10 conductivity [B, n_depth] (bin centres
 * ((v + 0.5) / n_value) 2 half_width - half_width + log_mean_prior[b] / ln 10; the q-point is the first bin whose cumulative share is >= q);
 * gbp_hitmap_runs -- the maps' rows (M = n_value * n_depth cells) in run-length form: first call with start == NULL writes the number
 * of runs of every row to counts[B]; the caller forms ptr[B + 1] (exclusive prefix) and calls again with ptr, start[ptr[B]], value[ptr[B]]
 * (run r of row b: value[ptr[b] + r] from cell start[ptr[b] + r] to the next run's start). */
gbp_status gbp_hitmap_statistics(int B, int n_value, int n_depth, const int32_t *hitmap, const double *log_mean_prior, double half_width,
                                 double *mean, double *p05, double *p50, double *p95, void *stream);
gbp_status gbp_hitmap_runs(int B, int64_t M, const int32_t *hitmap, int64_t *counts, const int64_t *ptr, int32_t *start, int32_t *value,
                           void *stream);
/* gbp_hitmap_products -- the per-column moments the line products (mode, percentiles, credible range, opacity, DOI, entropy:
 * geobipy_amd/line_products.py) derive from, each [B, n_depth]: mean as gbp_hitmap_statistics (the same bits); mode_idx = the first value
 * bin of the largest count (0 for an empty column); total = sum_v c (int64); s1 = sum_v c ln c (0 ln 0 = 0); and q_idx [n_q, B, n_depth] =
 * #{v : cumsum_v / max(total, 1) < q[k]} clamped to n_value - 1, the bin of quantile q[k] (q: a HOST array of n_q <= 8 values in (0, 1);
 * q_idx may be NULL when n_q == 0).  GBP_ERR_INVALID_ARG for bad sizes, NULL pointers or a q outside (0, 1). */
gbp_status gbp_hitmap_products(int B, int n_value, int n_depth, const int32_t *hitmap, const double *log_mean_prior, double half_width,
                               int n_q, const double *q, double *mean, int32_t *mode_idx, int32_t *q_idx, int64_t *total, double *s1,
                               void *stream);
/* gbp_hitmap_classes -- class (lithology) probabilities of every column for K classes in log10 conductivity (S/m), the reference's
 * Histogram.compute_probability(MvNormal(mean, variance), log=10, axis=0) (mesh/RectilinearMesh2D.py _compute_probability): with x_v the
 * bin centres of gbp_hitmap_statistics and w_k(x) = exp(-((x - means[k]) / scales[k])^2 / 2) / (sqrt(2 pi) scales[k]) (scipy's
 * norm.pdf -- scales[k] is a STANDARD DEVIATION: the reference hands the number it calls variance to scipy as scale),
 * prob[b, k, z] = sum_v c_v w_k(x_v) / sum_k' sum_v c_v w_k'(x_v) ([B, K, n_depth]; NaN where every term is 0, an empty column among
 * them); best[b, z] = the first class of the largest probability (numpy argmax; an all-NaN column: 0) and best_p[b, z] its probability
 * ([B, n_depth]).  means / scales: HOST arrays of K values, 1 <= K <= 16, means finite, scales finite and > 0; the table of K * n_value
 * fp64 weights lives in LDS and must fit in 64 KiB.  GBP_ERR_INVALID_ARG for bad sizes or classes, NULL pointers or B * n_depth beyond
 * int32, every check before any launch; B == 0 launches nothing. */
gbp_status gbp_hitmap_classes(int B, int n_value, int n_depth, const int32_t *hitmap, const double *log_mean_prior, double half_width, int K,
                              const double *means, const double *scales, double *prob, int32_t *best, double *best_p, void *stream);
/* gbp_hitmap_intervals -- interval marginals: out[b, v, m] = sum of hitmap[b, v, z] over the depth cells lo[b, m] <= z < hi[b, m], int64
 * [B, n_value, M] -- the reference's Histogram[:, lo:hi].marginalize(axis=1) (statistics/Histogram.py), the marginal posterior of a depth
 * or elevation unit, for M ranges at once.  lo / hi: DEVICE int32 [B, M], half-open, clamped to [0, n_depth] by the kernel, hi <= lo: no
 * cells (0); ranges may overlap and differ from sounding to sounding.  int64 because ten cells of a long chain's map sum beyond 2^31.
 * One streaming read of the maps; no atomics.  1 <= M <= 4096 and n_depth <= 1024 (the row prefix and the ranges live in LDS);
 * GBP_ERR_INVALID_ARG for the rest, for bad sizes and NULL pointers, every check before any launch; B == 0 launches nothing.
 * gbp_hitmap_products_i64 / gbp_hitmap_classes_i64 -- gbp_hitmap_products / gbp_hitmap_classes over int64 maps (such marginals, with
 * M in the place of n_depth): the same kernels instantiated on the count type, the same bits on the same counts (counts < 2^53). */
gbp_status gbp_hitmap_intervals(int B, int n_value, int n_depth, int M, const int32_t *hitmap, const int32_t *lo, const int32_t *hi,
                                int64_t *out, void *stream);
/* Two kernels on a finished posterior ensemble (gbp_rj_chains.ens_k, ens_edges, ens_sigma; csrc/gbp_ensemble.h):
 * gbp_ensemble_raster -- realisations on a depth axis: out[b, r, c] (f64 [B, R, n_depth]) = the conductivity of the layer of slot
 * slots[r] of chain b that holds z[c], layer = #{l < k - 1 : edges[l] <= z[c]} (the hit map's rule: an interface exactly at a cell
 * centre gives the layer below); a pure gather -- the stored double bit for bit; a whole row is NaN for an empty slot (ens_k == 0) or
 * a slot outside 0 .. n_ensemble - 1.  slots: DEVICE int32 [R], any order, repeats allowed; z: DEVICE [n_depth], the cell centres.
 * gbp_ensemble_rebin -- any posterior the sampler could have binned, after the fact: every filled slot, in order, with weight 1,
 * through the sampler's own accumulators (the same bits), into outputs the entry zeroes first: hitmap int32 [B, n_value, n_depth] on
 * the axes given (depth cell c spans [c, c + 1) depth_bin_width; NULL: none), unit_hist int32 [B, Q, n_value, n_units] of unit_z
 * [B, n_units, 2] (DEVICE), unit_kinds the bits of gbp_rj_options.unit_kinds; n_units == 0: none, first_hist int32 [B, n_first, n_depth] and first_none
 * [B, n_first] of first_threshold / first_direction (HOST arrays of n_first values; 0: none).  log_mean_prior: DEVICE [B].
 * Both: 1 <= n_ensemble <= 4096, 1 <= K <= 64; GBP_ERR_INVALID_ARG for bad sizes, axes, units or thresholds and NULL pointers, every
 * check before any launch; B == 0 launches nothing. */
gbp_status gbp_ensemble_raster(int B, int n_ensemble, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma, int R,
                               const int32_t *slots, int n_depth, const double *z, double *out, void *stream);
gbp_status gbp_ensemble_rebin(int B, int n_ensemble, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma,
                              const double *log_mean_prior, int n_value, double value_half_width, int n_depth, double depth_bin_width,
                              int32_t *hitmap, int n_units, int unit_kinds, const double *unit_z, int32_t *unit_hist, int n_first,
                              const double *first_threshold, const int32_t *first_direction, int32_t *first_hist, int32_t *first_none,
                              void *stream);
/* Chain diagnostics of regularly spaced series (csrc/gbp_ensemble_diag.h): did the chain run long enough, and how many independent
 * samples stand behind a posterior mean.  Per sounding b: M = seg_m[b] segments of equal length N = seg_n[b]; segment m covers rows
 * seg_start[b, m] .. seg_start[b, m] + N - 1 (inside 0 .. n_rows - 1: the caller's duty).  L = min(max_lag, N - 1), lowered by one if
 * even.  Per variable, with sums over a segment's rows: mean_m, d = x - mean_m, acov_m(l) = (1/N) sum_{t < N - l} d_t d_{t+l} (l = 0 .. L);
 * W = (1/M) sum_m acov_m(0) N/(N-1); gm = (1/M) sum_m mean_m; Bn = sum_m (mean_m - gm)^2 / (M - 1) (0 when M = 1); vp = W (N-1)/N + Bn;
 * rho_0 = 1, rho_l = 1 - (W - (1/M) sum_m acov_m(l) N/(N-1)) / vp; Geyer's initial monotone sequence on the pairs P_k = rho_2k + rho_2k+1:
 * S = prev = P_0, pairs = 1, then for k = 1 .. (L-1)/2 stop unless P_k > 0, else prev = min(prev, P_k), S += prev, pairs += 1;
 * tau = max(2 S - 1, 1 / log10(M N)); ess = M N / tau; rhat = sqrt(vp / W); sd = sqrt(vp); mcse = sqrt(vp / ess); mean = gm.
 * stats f64 [B, 6, V]: mean, sd, rhat, tau, ess, mcse; pairs int32 [B, V] (== (L + 1) / 2: the sum ran into the lag cap); rho NULL or
 * f64 [B, max_lag + 1, V], NaN beyond L.  M = 0 or N < 4: every output of the sounding NaN, pairs 0.  A variable whose used samples
 * are all one value (compared as stored): mean = it, sd = 0, the rest NaN, pairs 0; one with a non-finite used sample: all NaN, pairs 0.
 * gbp_series_diagnostics reads x f64 [B, n_rows, V]; gbp_ensemble_diagnostics rasters x[t, c] = log10 of the conductivity of the
 * layer of slot t that holds z[c] (the rule of gbp_ensemble_raster) on the fly.  1 <= max_lag <= 255, 1 <= M_max <= 16, n_rows and
 * n_slots <= 32 768, 1 <= K <= 64; GBP_ERR_INVALID_ARG for these and NULL pointers, every check before any launch, the entry named in
 * gbp_last_error; B == 0 launches nothing.  No atomics, one order of addition: a call repeats its own bits. */
gbp_status gbp_series_diagnostics(int B, int n_rows, int V, const double *x, int M_max, const int32_t *seg_start, const int32_t *seg_m,
                                  const int32_t *seg_n, int max_lag, double *stats, int32_t *pairs, double *rho, void *stream);
gbp_status gbp_ensemble_diagnostics(int B, int n_slots, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma,
                                    int n_depth, const double *z, int M_max, const int32_t *seg_start, const int32_t *seg_m,
                                    const int32_t *seg_n, int max_lag, double *stats, int32_t *pairs, double *rho, void *stream);
/* Ranks within the columns of such series (csrc/gbp_ensemble_ranks.h; the host statement of the rule is
 * geobipy_amd/ensembles.py rank_counts_reference): what rank-normalised R-hat, bulk / tail ESS, exact sample quantiles and Spearman's
 * correlation are made of.  Per sounding b the used rows are r_j = seg_start[b, m] + t, j = m N + t, of its M = seg_m[b] segments of
 * N = seg_n[b] rows (the lists of the diagnostics), n = M N of them; per variable v the column c_j = x[r_j, v]:
 *   order[b, i, 0, v] = s[lo_i], order[b, i, 1, v] = s[min(lo_i + 1, n - 1)], s = c sorted ascending, lo_i = floor((n - 1) p[i]) (one
 *   fp64 product) -- taken before any folding;
 *   fold != 0: med = 0.5 (s[(n - 1) / 2] + s[n / 2]), c_j <- |c_j - med| (a folded value may be +inf: it ranks as the largest);
 *   less[b, r_j, v] = #{i : c_i < c_j}, leq[b, r_j, v] = #{i : c_i <= c_j}: values compare as doubles (-0.0 equals +0.0), so
 *   0 <= less < leq <= n, and (less + leq + 1) / 2 is the midrank.
 * less, leq int32 [B, n_rows, V] (a pair), order f64 [B, n_p, 2, V], x_out f64 [B, n_rows, V]: the values that were ranked, before
 * folding, at the used rows (gbp_ensemble_ranks: log10 of the stored conductivity of the layer that holds z[v], the value
 * gbp_ensemble_diagnostics sees), NaN elsewhere; each of the three may be NULL and is then skipped.  A row in no segment: less = leq
 * = -1.  M = 0, N < 4 or M N > n_rows (overlapping segments): less = leq = -1 everywhere, order NaN.  A variable with a non-finite used
 * value: less = leq = -1 at the used rows, its order NaN.  p: HOST array of n_p probabilities.
 * 0 <= n_p <= 16, every p finite in [0, 1], n_rows and n_slots <= 16 384 (a padded column of doubles lives in LDS), 1 <= M_max <= 16,
 * 1 <= K <= 64, at most 2^32 - 1 threads; GBP_ERR_INVALID_ARG for these and NULL pointers, every check before any launch, the entry
 * named in gbp_last_error; B == 0 launches nothing.  A segment that leaves the rows is the caller's error: its rows are clamped.  No
 * atomics, every output has one writer: a call repeats its own bits. */
gbp_status gbp_series_ranks(int B, int n_rows, int V, const double *x, int M_max, const int32_t *seg_start, const int32_t *seg_m,
                            const int32_t *seg_n, int fold, int n_p, const double *p, int32_t *less, int32_t *leq, double *order,
                            double *x_out, void *stream);
gbp_status gbp_ensemble_ranks(int B, int n_slots, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma,
                              int n_depth, const double *z, int M_max, const int32_t *seg_start, const int32_t *seg_m,
                              const int32_t *seg_n, int fold, int n_p, const double *p, int32_t *less, int32_t *leq, double *order,
                              double *x_out, void *stream);
/* Weighted products within the columns of such series (csrc/gbp_ensemble_weighted.h; the host statement of the rule is
 * geobipy_amd/ensembles.py weighted_reference): the mean, sd, quantiles and exceedance weights of a sounding's models under weights --
 * the smoothed marginals of a section, a borehole's re-weighting, importance weights, dwell counts.
 * WEIGHTS ARE INTEGERS.  Model u < m = n_used[b] (clamped to 0 .. n) of sounding b is row rows[b, u] (rows int32 [B, n]; gbp_series_weighted: a
 * row of x f64 [B, n_rows, V]; gbp_ensemble_weighted: a slot) with multiplicity q[b, u] (int64 [B, n], 0 <= q <= 2^40; a value outside is
 * the caller's error and is clamped), so that sum q <= 2^52 and every decision below is a comparison of integers, or of integers exact
 * in fp64: no order of addition and no tie order can change a bit.  (ensembles.quantise_weights is the one documented step from
 * floating-point weights: q = rint(w / max w * 2^40).)
 *   x_u      gbp_series_weighted: x[b, rows[b, u], v]; gbp_ensemble_weighted: log10 of the stored conductivity of layer
 *            #{l < k - 1 : edges[l] <= z[v]} of the slot -- the expression of gbp_ensemble_ranks / gbp_ensemble_diagnostics.
 *   A row with q_u == 0 takes no part, whatever it holds or names: it is never loaded.  A participating row index outside the rows is
 *   the caller's error and is clamped before any load; a participating empty slot (k == 0) has the value NaN.
 *   total[b] = W = sum_u q_u (int64 [B]).  C(t) = sum_{u : x_u <= t} q_u, values compared as doubles (-0.0 equals +0.0).
 *   quantile[b, i, v] = the smallest participating value t with (double)C(t) >= max(p[i] * (double)W, 1.0) (one fp64 product): the inverse
 *            of the weighted ECDF, type 1; p = 0 gives the smallest value of positive weight.  With equal weights it is s[max(ceil(p n),
 *            1) - 1] of the sorted column -- NOT the interpolated pair of gbp_ensemble_ranks' order.
 *   above[b, j, v] = sum_{u : x_u >= thr[j]} q_u (int64): divided by W it is the exceedance probability.
 *   stats[b, 0, v] = mean = sum q x / W; stats[b, 1, v] = sd = sqrt(sum q (x - mean)^2 / W): two passes in fp64 (tied values enter with
 *            their summed weight; the order of addition is fixed, so a call repeats its bits, but it is not part of the rule).
 *   W == 0: quantile, mean and sd NaN, above 0.  A column with a non-finite participating value: quantile, mean, sd NaN, above -1.
 * quantile f64 [B, n_p, V], above int64 [B, n_t, V], stats f64 [B, 2, V]: each may be NULL and is then skipped.  p: HOST array of n_p
 * probabilities, thr: HOST array of n_t thresholds (gbp_ensemble_weighted: log10 S/m).
 * 1 <= n <= 4096 (keys and bins of a padded column live in LDS), n_rows / n_slots >= 1, V / n_depth >= 1, 1 <= K <= 64, 0 <= n_p <= 16 with
 * every p finite in [0, 1], 0 <= n_t <= 8 with every thr finite, at most 2^32 - 1 threads; GBP_ERR_INVALID_ARG for these and NULL pointers,
 * every check before any launch, the entry named in gbp_last_error; B == 0 launches nothing.  No global atomics, every output has one
 * writer, the additions in LDS are of integers: a call repeats its own bits. */
gbp_status gbp_series_weighted(int B, int n_rows, int V, const double *x, int n, const int32_t *rows, const int32_t *n_used, const int64_t *q,
                               int n_p, const double *p, int n_t, const double *thr, int64_t *total, double *quantile, int64_t *above,
                               double *stats, void *stream);
gbp_status gbp_ensemble_weighted(int B, int n_slots, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma,
                                 int n_depth, const double *z, int n, const int32_t *rows, const int32_t *n_used, const int64_t *q,
                                 int n_p, const double *p, int n_t, const double *thr, int64_t *total, double *quantile, int64_t *above,
                                 double *stats, void *stream);
/* Correlation between the variables of such series (csrc/gbp_ensemble_corr.h): what moves together.  Per sounding b
 * the used rows are those of its M = seg_m[b] segments of N = seg_n[b] rows (the lists of the diagnostics), n = M N of them:
 * mu_v = (1/n) sum_t x_tv; d_tv = x_tv - mu_v; C(u, v) = (1/(n - 1)) sum_t d_tu d_tv (the pooled sample covariance); sd_v = sqrt(C(v, v));
 * R(u, v) = C(u, v) / (sd_u sd_v).  stats f64 [B, 2, V]: mean, sd; band f64 [B, V, W + 1], W = band_width, j fastest:
 * band[b, c, j] = R(c, c + j) (normalise != 0) or C(c, c + j) (normalise == 0), NaN where c + j >= V.  M = 0 or n < 4: everything NaN.
 * A variable whose used samples are all one value (compared as stored): mean = it, sd = 0, every band entry that involves it NaN, its
 * own diagonal included; one with a non-finite used sample: mean, sd and its entries NaN; no other entry is touched by either.  R of
 * a live variable with itself is 1.0 exactly (written, not computed).  sd is the pooled sample standard deviation; the diagnostics'
 * sd = sqrt(vp) differs from it by O(1/N).  The products are of centred values, accumulated in fp64 (v_mfma_f64_16x16x4_f64).
 * gbp_series_correlation reads x f64 [B, n_rows, V]; gbp_ensemble_correlation rasters x[t, c] as gbp_ensemble_diagnostics does.
 * gbp_band_runs: from a band and a threshold, per cell c, down[c] = the number of consecutive j = 1, 2, ... with j <= W, c + j <= V - 1
 * and band[c, j] >= threshold (NaN compares false and ends the run); up[c] the same with band[c - j, j], c - j >= 0; closed uint8
 * [B, 2, V] = closed_up, closed_down: 1 iff the walk ended at an entry not >= threshold (0: it ended at j = W or at the end of the
 * axis).  A cell whose diagonal is NaN: up = down = 0, closed 0.
 * 1 <= V, 0 <= band_width <= V - 1, n_rows and n_slots <= 32 768, 1 <= M_max <= 16, 1 <= K <= 64; GBP_ERR_INVALID_ARG for these and
 * NULL pointers, every check before any launch, the entry named in gbp_last_error; B == 0 launches nothing.  A segment that leaves the
 * rows is the caller's error: its rows are clamped.  No atomics, one order of addition: a call repeats its own bits. */
gbp_status gbp_series_correlation(int B, int n_rows, int V, const double *x, int M_max, const int32_t *seg_start, const int32_t *seg_m,
                                  const int32_t *seg_n, int band_width, int normalise, double *stats, double *band, void *stream);
gbp_status gbp_ensemble_correlation(int B, int n_slots, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma,
                                    int n_depth, const double *z, int M_max, const int32_t *seg_start, const int32_t *seg_m,
                                    const int32_t *seg_n, int band_width, int normalise, double *stats, double *band, void *stream);
gbp_status gbp_band_runs(int B, int V, int band_width, const double *band, double threshold, int32_t *up, int32_t *down, uint8_t *closed,
                         void *stream);
/* Families of kept models (csrc/gbp_ensemble_families.h; the host statements of the rules are geobipy_amd/families.py
 * distance_reference and families_reference): which sampled model is representative, and is the posterior one family of models or several.
 * gbp_ensemble_distance -- model u of sounding b is slot rows[b, u] of the ensemble (rows int32 [B, n]): k layers, interfaces e[0 .. k - 2]
 * ascending, values a[l] = log10 sigma[l] (log10 != 0) or the stored doubles (log10 == 0); its value at depth z is that of layer
 * #{l < k - 1 : e[l] <= z} (the count of gbp_ensemble_raster: an interface exactly at z gives the layer below).  On the window [z0, z1]
 * with the measure mu([p, q]) = q - p (measure 0, linear) or ln(q / p) (measure 1, log; z0 > 0):
 *   D2(u, v) = (1 / mu([z0, z1])) sum over the merged segments [p, q) of mu([p, q]) (a_u(p) - a_v(p))^2,  D = sqrt(D2),
 * the breakpoints being z0, every interface of either model strictly inside (z0, z1) in ascending order, and z1: the exact integral of
 * the squared difference of two piecewise-constant functions, O(k_u + k_v) per pair and no depth axis.  dist f64 [B, n, n] holds D
 * (squared == 0) or D2; dist[b, u, v] and dist[b, v, u] are one value, bit for bit; the diagonal of a present model is 0.0 (written, not
 * computed) and two slots that hold one model are exactly 0 apart.  A row outside 0 .. n_slots - 1 or a slot with k <= 0 is absent: its
 * row, column and diagonal are NaN (the slot index is clamped before any load).
 * gbp_distance_families -- k-medoids on dist, per sounding on its first m = n_used[b] models (clamped to 0 .. n), stages q = 1 .. q_max;
 * every sum runs over j = 0 .. m - 1 in ascending order in fp64.  If an entry of dist[b, :m, :m] is non-finite or negative, or m == 0:
 * n_found = 0 and every stage is not found.  Stage 1: the medoid is argmin_i sum_j dist[j, i].  Stage q > 1: stage q - 1's final medoids
 * plus the candidate c with the greatest gain sum_j max(nearest[j] - dist[j, c], 0) against stage q - 1's final assignment; a greatest gain
 * of 0.0 means fewer than q distinct models: this stage and the later ones are not found, n_found = q - 1.  Then at most max_iter times:
 * assign every model j to the medoid c_p with the least dist[c_p, j] (ties to the medoid that joined first); per family the new medoid is
 * the member i with the least sum_{j in the family} dist[j, i] (a family without a member keeps its medoid); no medoid changed:
 * converged = 1, stop.  When the cap is reached the models are assigned once more to the current medoids and converged = 0.  iterations
 * counts the updates.  Every argmin / argmax takes the lowest index among equals.  Per stage: medoid int32 [B, q_max, q_max] (indices into
 * the model list; -1 beyond q), label int32 [B, q_max, n] (the medoid's position; -1 for j >= m), nearest and second f64 [B, q_max, n] (the
 * distances to the nearest and the second-nearest medoid: copies of dist entries; second is NaN at stage 1), iterations int32 and converged
 * uint8 [B, q_max]; n_found int32 [B].  A stage not found: -1, -1, NaN, NaN, 0, 0.  Every output is an integer or a copy of an input double.
 * 1 <= n <= 4096, 1 <= K <= 64, 1 <= q_max <= 8, max_iter >= 0, finite 0 <= z0 < z1, z0 > 0 for the log measure; GBP_ERR_INVALID_ARG for
 * these, for NULL pointers and for a launch of more than 2^32 - 1 threads (256 per tile pair, 256 per sounding), every check before any launch, the entry named in gbp_last_error;
 * B == 0 launches nothing.  No atomics, one order of addition: a call repeats its own bits. */
gbp_status gbp_ensemble_distance(int B, int n_slots, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma,
                                 int n, const int32_t *rows, double z0, double z1, int measure, int log10, int squared, double *dist,
                                 void *stream);
gbp_status gbp_distance_families(int B, int n, const double *dist, const int32_t *n_used, int q_max, int max_iter, int32_t *medoid,
                                 int32_t *label, double *nearest, double *second, int32_t *iterations, uint8_t *converged, int32_t *n_found,
                                 void *stream);
/* gbp_ensemble_cross_distance -- the distance of gbp_ensemble_distance, word for word (the same breakpoints, the same order of the sum,
 * the same log1p: one device function serves both kernels, so a pair of models gives the same bits through either entry), between the
 * models of DIFFERENT soundings (the host statement is geobipy_amd/sections.py cross_distance_reference).  rows int32
 * [S, n] as above; partner int32 [S]: the sounding that sounding s is paired with, or -1.  dist f64 [S, n, n]: dist[s, i, j] is D (or
 * D2) between model rows[s, i] of sounding s and model rows[partner[s], j] of sounding partner[s].  An absent model (a row outside
 * 0 .. n_slots - 1, a slot with k <= 0) gives NaN in its row (i) or column (j); a sounding whose partner is -1 or otherwise outside
 * 0 .. S - 1 gets a slab of NaN.  Every entry is written.  Nothing is symmetric and there is no diagonal: i and j are models of
 * different soundings, and two identical models are exactly 0.0 apart by arithmetic.  One workgroup of 256 threads per (sounding,
 * 16 x 16 tile), all nt x nt tiles.  The limits and refusals of gbp_ensemble_distance (256 threads per tile; a NULL partner); S == 0
 * launches nothing.  No atomics: a call repeats its own bits. */
gbp_status gbp_ensemble_cross_distance(int S, int n_slots, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma,
                                       int n, const int32_t *rows, const int32_t *partner, double z0, double z1, int measure, int log10,
                                       int squared, double *dist, void *stream);
gbp_status gbp_hitmap_products_i64(int B, int n_value, int n_depth, const int64_t *hitmap, const double *log_mean_prior, double half_width,
                                   int n_q, const double *q, double *mean, int32_t *mode_idx, int32_t *q_idx, int64_t *total, double *s1,
                                   void *stream);
gbp_status gbp_hitmap_classes_i64(int B, int n_value, int n_depth, const int64_t *hitmap, const double *log_mean_prior, double half_width,
                                  int K, const double *means, const double *scales, double *prob, int32_t *best, double *best_p,
                                  void *stream);
/* gbp_hitmap_pool -- replicate chains (no reference counterpart, the host statement of the rule is
 * geobipy_amd/replicates.py pool_reference): hitmap holds S * C maps, row s * C + c the replicate c of sounding s; use: DEVICE int32
 * [S, C], non-zero = the chain takes part.  With x_v the bin centres of gbp_hitmap_statistics WITHOUT the prior shift and per chain
 * n_c = sum_v h (int64), a_c = sum_v h x_v, q_c = sum_v (h x_v) x_v, e_c = sum_{h > 0} h ln h (fp64, v ascending), per depth cell:
 * pooled [S, n_value, n_depth] = sum_{c: use} h_c;  n_used [S, n_depth] = m = |P|, P = {c: use and n_c > 0};
 * chain_mean [S, C, n_depth] = m_c = a_c / n_c (NaN outside P);
 * rhat [S, n_depth] = sqrt(((nbar - 1) / nbar W + Bn) / W), the Gelman-Rubin potential scale reduction, with W = sum_P s2_c / m,
 * s2_c = max(0, (q_c - a_c m_c) / (n_c - 1)) (0 when n_c < 2), Bn = sum_P (m_c - mbar)^2 / (m - 1), mbar = sum_P m_c / m,
 * nbar = N_P / m, N_P = sum_P n_c; W == 0: 1 when Bn == 0, else +inf;
 * jsd [S, n_depth] = max(0, [(ln N_P - e_p / N_P) - sum_P (n_c / N_P)(ln n_c - e_c / n_c)] / ln 2), e_p = sum_{hp > 0} hp ln hp of
 * the pooled column: the generalised Jensen-Shannon divergence of the chains' columns in bits (0: identical, log2 m: disjoint).
 * rhat and jsd are NaN when m < 2; sums over P run in ascending c.  The axis is generic: a [rows, cells] histogram is a map with
 * n_depth = 1.  2 <= C <= 8; GBP_ERR_INVALID_ARG for the rest, for bad sizes, NULL pointers and S * n_depth beyond int32, every check
 * before any launch; S == 0 launches nothing.  The caller keeps C times a column's total below 2^31. */
gbp_status gbp_hitmap_pool(int S, int C, int n_value, int n_depth, const int32_t *hitmap, const int32_t *use, double half_width,
                           int32_t *pooled, int32_t *n_used, double *chain_mean, double *rhat, double *jsd, void *stream);
/* gbp_hitmap_mixture -- local mixture fits (the host statement of the rule is geobipy_amd/mixtures.py
 * mixture_reference): for every column, every stage K = 1 .. Kmax in one launch -- K Gaussians fitted to the binned column (cell centres
 * x_v of gbp_hitmap_statistics WITHOUT the prior shift, dx = 2 half_width / n_value) by n_iter EM iterations on the cells with counts,
 * sums over v ascending: start w_j = 1 / K, mu_j = the centre of the first cell with 2 K cum_v >= (2 j + 1) N, s2_j = V / K^2 + reg (m, V
 * the column's mean and variance); E-step l_vj = ln w_j - ln(2 pi s2_j) / 2 - (x_v - mu_j)^2 / (2 s2_j), L_v = logsumexp_j l_vj,
 * r_vj = c_v exp(l_vj - L_v); M-step about the old mean d = x_v - mu_j: n_j = sum r + 10 * 2^-52, A = sum r d, Q = sum r d^2,
 * mu_j += A / n_j, s2_j = max(Q / n_j - (A / n_j)^2, 0) + reg, w_j = n_j / sum_j n_j.  Stage 1 is the closed form (1, m, V + reg).
 * A closing pass over ALL cells gives loglik = sum c_v L_v / N, ll_change = loglik minus that of the last E-step (0 at stage 1) and,
 * with f_v = exp(L_v) dx and p_v = c_v / N, misfit = (max |p - f| / max p, ||p - f||_2 / ||p||_2).
 * weight / mean / sd (= sqrt s2): [B, Kmax (Kmax + 1) / 2, n_depth], stage K in slots K (K - 1) / 2 .. + K; loglik / ll_change:
 * [B, Kmax, n_depth]; misfit: [B, Kmax, 2, n_depth].  An empty column: NaN everywhere.  1 <= Kmax <= 4, 1 <= n_iter <= 10 000, reg and
 * half_width finite and > 0, n_value <= 4096; GBP_ERR_INVALID_ARG for the rest, for bad sizes, NULL pointers and B * n_depth beyond int32, every check
 * before any launch; B == 0 launches nothing.  gbp_hitmap_mixture_i64: the same over int64 maps (interval marginals). */
gbp_status gbp_hitmap_mixture(int B, int n_value, int n_depth, const int32_t *hitmap, double half_width, int Kmax, int n_iter, double reg,
                              double *weight, double *mean, double *sd, double *loglik, double *ll_change, double *misfit, void *stream);
gbp_status gbp_hitmap_mixture_i64(int B, int n_value, int n_depth, const int64_t *hitmap, double half_width, int Kmax, int n_iter, double reg,
                                  double *weight, double *mean, double *sd, double *loglik, double *ll_change, double *misfit, void *stream);

/* [host] Results containers (geobipy_amd/h5lite.py; no reference counterpart -- the reference stores its hit maps dense): the rows of
 * a conductivity-depth hit map held as runs (row r owns runs ptr[r] .. ptr[r + 1] - 1; run q holds value[q] from cell start[q] of the row
 * -- the first at 0 -- to the next run's start) -> one zlib stream of the row's dense int32 bytes per row, written from the runs
 * (csrc/gbp_hostpack.h): out[out_ptr[r] .. out_ptr[r + 1]).  Capacity: 16 bytes per run + cells_per_row / 32 + 64 per row is enough. */
gbp_status gbp_runs_to_zlib(int n_rows, int64_t cells_per_row, const int64_t *ptr, const int32_t *start, const int32_t *value,
                            uint8_t *out, int64_t out_capacity, int64_t *out_ptr);

/* Survey volumes: discrete Sibson (natural-neighbour) gridding of per-sounding columns onto a regular x-y raster (csrc/gbp_grid.h), the
 * reference's method='sibson' (base/interpolation.py __sibson_2d_inner), split into a plan (geometry, once per grid) and an apply (once
 * per block of columns).  px / py [N]: DEVICE arrays of the soundings' pixel coordinates ((x - x_edges[0]) / dx, (y - y_edges[0]) / dy).
 * Pixel (i, j), 0 <= i < ny, 0 <= j < nx: index = the sounding nearest to the node (j, i) (lowest index on a tie),
 * D = int(ceil(sqrt((j - px)^2 + (i - py)^2))) (capped at 2^30); it covers pixel (i_s, j_s) iff i - D <= i_s < i + D, j - D <= j_s < j + D
 * and (i_s - i)^2 + (j_s - j)^2 <= D^2 + 0.25; n = the number of pixels covering a pixel.
 * gbp_sibson_apply: out[c, i_s, j_s] = (sum of values[index[i, j], c] over the covering (i, j) in row-major order, from 0.0) / n
 * (n = 0: NaN), NaN where the pixel's own D^2 + 0.25 > max_distance_px2 (+inf: no mask); values [N, C] row-major and out [C, ny, nx]
 * on the plan's device, fp64.  The order of the sum is fixed, so results are bitwise reproducible.
 * The lists hold sum(n) int32 entries.  Beyond list_budget_bytes (0: 4 GiB) the plan keeps room for one band of destination rows
 * and gbp_sibson_apply rewrites it band by band (same results; such a plan serves one apply at a time).
 * gbp_sibson_plan_create synchronises the stream.  gbp_sibson_plan_query copies index / distance / count ([ny, nx] int32 DEVICE arrays,
 * each may be NULL) on the stream and fills the HOST array info[4] (may be NULL) = {sum(n), max(n), number of bands, device bytes held}.
 * GBP_ERR_INVALID_ARG: N < 1, nx or ny < 1, nx * ny beyond int32, NULL pointers, a non-finite pixel coordinate, NaN max_distance_px2,
 * a row of lists beyond the budget, C < 1, C * nx * ny or N * C out of range. */
typedef struct gbp_sibson_plan gbp_sibson_plan;
gbp_status gbp_sibson_plan_create(int N, const double *px, const double *py, int nx, int ny, double max_distance_px2, void *stream,
                                  gbp_sibson_plan **out);
gbp_status gbp_sibson_plan_create_ex(int N, const double *px, const double *py, int nx, int ny, double max_distance_px2,
                                     int64_t list_budget_bytes, void *stream, gbp_sibson_plan **out);
void gbp_sibson_plan_destroy(gbp_sibson_plan *plan);
gbp_status gbp_sibson_plan_query(const gbp_sibson_plan *plan, int32_t *index, int32_t *distance, int32_t *count, int64_t *info, void *stream);
gbp_status gbp_sibson_apply(const gbp_sibson_plan *plan, int C, const double *values, double *out, void *stream);

/* Pixel posteriors (csrc/gbp_grid.h k_sibson_pool; no reference counterpart: the reference grids finished products): the linear pool
 * of the hit maps of each listed pixel's natural neighbours, with the plan's lists as they are.  pixels [n_pixels] int32 flat pixel
 * numbers (i * nx + j; any order, repeats allowed), maps [N, n_value, n_depth] int32 (N the plan's soundings, depth fastest), u [N] fp64
 * or NULL, pooled [n_pixels, n_value, n_depth] int32, clipped [n_pixels, n_depth] int64 or NULL: DEVICE arrays on the plan's device.
 * For pixel p = pixels[i] with nearest sounding r = index[p] and list entries s_e:
 *   d_e = 0 without u, else (int) rint(u[s_e] - u[r]) (one fp64 subtraction, round half to even, clamped to +-n_value): u is a
 *   sounding's axis offset in value cells, so a neighbour's counts move by whole cells onto the nearest sounding's axis;
 *   pooled[i, v, c] = sum over e of maps[s_e, v - d_e, c] where 0 <= v - d_e < n_value;
 *   clipped[i, c] = sum over e of the counts of maps[s_e, :, c] whose row fell outside that range.
 * A pixel under the plan's mask (D^2 + 0.25 > max_distance_px2) or with an empty list gives zeros in both.  An entry adds its
 * sounding's counts as they are: more samples weigh more, an empty map weighs nothing.  Integer sums: exact, whatever the order.
 * The caller guarantees 0 <= pixels[i] < nx * ny (the list is not read on the host; the kernel gives zeros for a number outside).
 * max_total: the caller's bound of the largest column total of any map; a pooled cell is at most (longest list) * max_total.
 * GBP_ERR_INVALID_ARG, before any launch: n_pixels < 0, n_value or n_depth < 1, n_depth > 2^29, max_total < 0, a NULL plan, NULL
 * pixels / maps / pooled, a banded plan (n_bands > 1: its lists are not resident), (longest list) * max_total > 2^31 - 1, sizes out
 * of range.  n_pixels == 0 launches nothing. */
gbp_status gbp_sibson_pool(const gbp_sibson_plan *plan, int n_pixels, const int32_t *pixels, int n_value, int n_depth, const int32_t *maps,
                           const double *u, int64_t max_total, int32_t *pooled, int64_t *clipped, void *stream);

/* Elevation slices: rows on the depth-below-surface axis resampled onto an elevation axis (csrc/gbp_elev.h), the reference's
 * Inference2D.elevationSlice for every row and every elevation at once.  values [R, n_depth] row-major, surface [R / K] (row r belongs
 * to sounding r / K: [N, K, n_depth] class probabilities pass as R = N K rows), depth_edges [n_depth + 1] increasing, all fp64 DEVICE
 * arrays.  cell(d) = clamp(upper_bound(depth_edges, d) - 1, 0, n_depth - 1).
 * GBP_ELEVATION_LEVELS: axis = levels [E]; d = surface - level; out = values[cell(d)] when depth_edges[0] < d < depth_edges[n_depth]
 * (both strict), else NaN.  GBP_ELEVATION_INTERVALS: axis = edges [E + 1], cell k = (edges[k], edges[k + 1]); d0 = surface - edges[k],
 * d1 = surface - edges[k + 1]; out = the mean of values[cell(d1) .. cell(d0)] when d1 < depth_edges[n_depth] and d0 > depth_edges[0]
 * (an interval that only overlaps the mesh averages the cells it overlaps), NaN otherwise and for an empty range.  The mean is
 * sum / count with the sum in numpy's pairwise order (blocks of at most 128 terms on eight accumulators, halves split at multiples of
 * eight), so results equal the reference's in every bit and are reproducible.  A NaN surface gives NaN; NaN values propagate.
 * out [R, c1 - c0] row-major holds the columns c0 <= k < c1 of the axis: the [N, C] layout gbp_sibson_apply reads.
 * The axes are not read on the host: whether they are finite and increasing is the caller's to check.
 * GBP_ERR_INVALID_ARG: an unknown mode, R < 1, K < 1 or R % K != 0, n_depth < 1 or > 8191, E < 1, a window outside 0 <= c0 < c1 <= E,
 * NULL pointers, R * n_depth or R * (c1 - c0) out of range. */
#define GBP_ELEVATION_LEVELS 0
#define GBP_ELEVATION_INTERVALS 1
gbp_status gbp_elevation_resample(int mode, int R, int K, int n_depth, const double *values, const double *surface,
                                  const double *depth_edges, int E, const double *axis, int c0, int c1, double *out, void *stream);

/* Horizon tracking along lines (csrc/gbp_horizon.h k_horizon_viterbi, k_horizon_marginals; no reference counterpart: the rule is
 * stated in numpy as horizons.track_reference): the most probable path and the smoothed marginals of a Markov chain over the S depth
 * cells of a window (uniform width dz, ascending depth) and, where absent_score is given, the extra state "absent" (index S).
 * L sequences (a line, or a line x a horizon) are concatenated: ptr [L + 1] int64, sequence l holds the rows ptr[l] .. ptr[l + 1] - 1.
 * score [total_n, S], absent_score [total_n] or NULL (no absent state), g, d [total_n] (of the step n -> n + 1; the entry of a
 * sequence's last row is unused), all fp64 and finite; DEVICE arrays, ptr included: it is not read on the host, the caller passes
 * total_n = ptr[L] and max_n = the longest sequence, and guarantees that ptr starts at 0 and grows by at least 1.
 *   T_n[k] = g[n] * fabs(d[n] - (double)k * dz), k = c' - c: cell c under row n to cell c' under row n + 1; cell <-> absent costs
 *   switch_cost >= 0; absent -> absent costs 0.
 *   Viterbi: V_0 = score[0] (and absent_score[0]); V_{n+1}[c'] = score[n + 1, c'] + max(max_c (V_n[c] - T_n[c' - c]), V_n[S] -
 *   switch_cost); V_{n+1}[S] = absent_score[n + 1] + max(max_c (V_n[c] - switch_cost), V_n[S]).  The maximiser is the first maximum in
 *   the order c = 0 .. S - 1, then absent (strict > replaces) and is kept as a back-pointer; the path ends at the first maximum of
 *   V_{N-1} in the same order.  Every operation is one fp64 add, subtract, multiply or compare as written, so cell and log_score
 *   equal the numpy rule's in every bit.  cell [total_n] int32 (S: absent), log_score [L].
 *   Marginals (only when marginal, log_partition and scale are given: otherwise the second kernel is not launched): w = exp(score),
 *   K_n[k] = exp(-T_n[k]), ks = exp(-switch_cost); alpha_0 = w_0 / s_0; alpha_{n+1}[c'] = w[n + 1, c'] (sum_c alpha_n[c] K_n[c' - c]
 *   + alpha_n[S] ks), c ascending, the absent row sum_c alpha_n[c] ks + alpha_n[S], each normalised by its sum s_{n+1};
 *   beta_{N-1} = 1, beta_n = K_n (w_{n+1} o beta_{n+1}) / s_{n+1}; marginal [total_n, S + 1 or S] = alpha_n o beta_n renormalised
 *   (the absent state last, present only with absent_score); scale [total_n] = s_n; log_partition [L] = sum_n ln s_n.  The device's
 *   exp and the order of its normalising sums differ from numpy's: a few ulp.  Where every transition of a step underflows the
 *   marginals of the sequence are NaN (the path is not affected).
 * back: a workspace of total_n * (S + 1) uint16 (the back-pointers; followed on the device).  One 256-thread workgroup per sequence;
 * LDS: (4 S + 6) doubles.
 * GBP_ERR_INVALID_ARG, before any launch: L < 0, S < 1 or S > 2048, dz not positive, switch_cost negative or not finite, total_n <
 * L, max_n < 1 or > total_n, L * max_n < total_n, sizes out of range, a NULL ptr / score / g / d / back / cell / log_score, marginal,
 * log_partition and scale not all given or all NULL.  L == 0 launches nothing. */
gbp_status gbp_horizon_track(int L, const int64_t *ptr, int64_t total_n, int max_n, int S, double dz, const double *score,
                             const double *absent_score, const double *g, const double *d, double switch_cost, uint16_t *back,
                             int32_t *cell, double *log_score, double *marginal, double *log_partition, double *scale, void *stream);

/* Horizon pairs: the top and the base of one unit tracked jointly and ordered (csrc/gbp_horizon_unit.h k_unit_viterbi,
 * k_unit_marginals; the rule is stated in numpy as horizons.unit_reference).  The conventions of gbp_horizon_track:
 * L sequences concatenated by ptr [L + 1] int64 (a sequence has >= 1 row), DEVICE arrays, ptr included; the caller passes total_n =
 * ptr[L] and max_n.  The state under a row is a pair (a, b) of cells of one window of S <= 96 cells, valid when b - a >= min_cells
 * (0 .. S - 1), or, where absent_score is given, "absent".  score_top, score_base f64 [total_n, S]; thickness_score f64 [S] or NULL
 * (the term is left out); absent_score f64 [total_n] or NULL; g, d f64 [total_n] and dz, switch_cost as gbp_horizon_track takes them.
 *   Node: s[n, a, b] = (score_top[n, a] + score_base[n, b]) + thickness_score[b - a].  Step: T_n[k] = g[n] * fabs(d[n] - (double)k *
 *   dz); pass 1 M1[a', b] = max over a ascending of V[a, b] - T[a' - a]; pass 2 M2[a', b'] = max over b ascending of M1[a', b] -
 *   T[b' - b]; then V[absent] - switch_cost; every maximum is the first (strict > replaces).  V'[a', b'] = s[n + 1, a', b'] + M2;
 *   V'[absent] = absent_score[n + 1] + the first maximum of V[a, b] - switch_cost over the valid pairs in row-major order, then
 *   V[absent].  The path ends at the first maximum of the last V in row-major order, then absent.  cell_top, cell_base int32
 *   [total_n] (both S: absent) and log_score [L] equal the numpy rule's in every bit.
 *   Marginals (only when alpha .. scale are given): the same two passes as sums in the linear domain, scaled forward-backward;
 *   marginal_top, marginal_base, marginal_thickness (indexed by b - a) f64 [total_n, S], marginal_absent, scale f64 [total_n],
 *   log_partition f64 [L].  The normalising sums, the absent state's sums and the projections of gamma reduce in the device's order.
 * Workspaces: back uint8 [2, total_n, S, S]; back_absent int32 [total_n] (needed with absent_score); alpha f64 [total_n, S * S + 1]
 * (with the marginals).  One 512-thread workgroup per sequence; LDS: (2 S^2 + 5 S + 1040) doubles.
 * GBP_ERR_INVALID_ARG, before any launch: L < 0, S < 1 or S > 96, min_cells outside 0 .. S - 1, dz not positive, switch_cost negative
 * or not finite, total_n < L, max_n < 1 or > total_n, L * max_n < total_n, sizes out of range, a NULL ptr / score_top / score_base /
 * g / d / back / cell_top / cell_base / log_score, back_absent NULL with absent_score, alpha, the four marginals, log_partition and
 * scale not all given or all NULL.  L == 0 launches nothing. */
gbp_status gbp_horizon_unit_track(int L, const int64_t *ptr, int64_t total_n, int max_n, int S, int min_cells, double dz,
                                  const double *score_top, const double *score_base, const double *thickness_score,
                                  const double *absent_score, const double *g, const double *d, double switch_cost, uint8_t *back,
                                  int32_t *back_absent, int32_t *cell_top, int32_t *cell_base, double *log_score, double *alpha,
                                  double *marginal_top, double *marginal_base, double *marginal_thickness, double *marginal_absent,
                                  double *log_partition, double *scale, void *stream);

/* Sections of sampled models along lines (csrc/gbp_section.h k_section_viterbi, k_section_marginals; the rule is
 * stated in numpy as sections.track_reference): the most probable path and the smoothed marginals of a Markov chain whose states
 * under row r are the first m_r = n_used[r] (1 .. n) of n kept models and whose transition is a dense matrix per step.  The
 * conventions of gbp_horizon_track: L sequences concatenated by ptr [L + 1] int64 (a sequence has >= 1 row), DEVICE arrays, ptr
 * included; the caller passes total_n = ptr[L].  score f64 [total_n, n], g f64 [total_n], d2 f64 [total_n, n, n] of the step r ->
 * r + 1 (the entry of a sequence's last row is never read; nothing outside the prefixes i < m_r, j < m_{r+1} is read).
 *   Viterbi: V_0[j] = score[r0, j], j < m_0.  Per step and per j < m_{r+1}: best = -inf, arg = 0; for i = 0 .. m_r - 1 ascending
 *   cand = V[i] - g[r] * d2[r, i, j] (one fp64 multiply, one subtract), replaced on strict cand > best -- a NaN never wins --;
 *   V'[j] = score[r + 1, j] + best, back[r + 1, j] = arg.  The path ends at the first maximum of V over j < m_last: log_score [L]; the
 *   walk back gives state int32 [total_n], every state < m_r.  state and log_score equal the numpy rule's in every bit.
 *   Marginals (only when marginal, log_partition and scale are given): w = exp(score); alpha_0 = w_0 / s_0; u[j] = sum_i alpha[i]
 *   exp(-(g[r] d2[r, i, j])), i ascending; u <- w_{r+1} o u; s_{r+1} = sum u; alpha' = u / s_{r+1}; beta_last = 1, beta_r[i] = sum_j
 *   exp(-(g[r] d2[r, i, j])) w_{r+1}[j] beta_{r+1}[j] / s_{r+1}; marginal [total_n, n] = alpha o beta renormalised per row, 0.0 for
 *   the states >= m_r; scale [total_n] = s; log_partition [L] = sum ln s.  The device's exp and the order of its normalising and
 *   backward sums differ from numpy's: a few ulp.  Where every transition of a step underflows the marginals of the sequence are NaN
 *   (the path is not affected).
 * back: a workspace of total_n * n uint16.  One 256-thread workgroup per sequence; LDS: (2 n + 4) doubles, 3 KiB static.
 * GBP_ERR_INVALID_ARG, before any launch: L < 0, n < 1 or n > 1024, total_n < L, sizes out of range, a NULL ptr / n_used / score / g /
 * d2 / back / state / log_score, marginal, log_partition and scale not all given or all NULL.  L == 0 launches nothing. */
gbp_status gbp_section_track(int L, const int64_t *ptr, int64_t total_n, int n, const int32_t *n_used, const double *score,
                             const double *g, const double *d2, uint16_t *back, int32_t *state, double *log_score, double *marginal,
                             double *log_partition, double *scale, void *stream);

/* Joint draws of whole sections from the chain of gbp_section_track by forward filtering and backward sampling (csrc/gbp_section.h
 * k_section_filter, k_section_draw; the rule is stated in numpy as sections.draw_reference).  L, ptr, total_n, n,
 * n_used, score, g, d2 as above, with one difference: a sequence may be empty (ptr repeated; nothing is written for it).
 *   Filter: the forward pass of the marginals above, by the same device function: filtered f64 [total_n, n] = alpha_r, 0.0 for the
 *   states >= m_r; scale [total_n] = s_r, a workspace the caller provides.
 *   Draws: realisation rho = 0 .. n_draws - 1 walks r = last .. first of every sequence.  W[i] = alpha_r[i] at the last row, alpha_r[i]
 *   * exp(-(g[r] * d2[r, i, j])) elsewhere, j the state just drawn under r + 1; c[i] = c[i - 1] + W[i] for i = 0 .. m_r - 1 ascending;
 *   thr = u * c[m_r - 1]; the state is min(#{i : c[i] <= thr}, m_r - 1): a state of weight 0 is never drawn, and with a NaN total no
 *   comparison holds and the state is 0.  u = u53(x, y) of Philox4x32-10 with key seed and counter (rho, key & 0xFFFFFFFF, key >> 32,
 *   0), key = row_key[r] (int64 [total_n]; NULL: r): a draw depends on the seed, the realisation and the row's key, not on n_draws nor
 *   on how sequences are grouped into launches.  draw_state int32 [n_draws, total_n], every state < m_r.  The device's exp is not
 *   numpy's to the last bit: a draw whose threshold lies within rounding of a c[i] may fall either way, and the walk differs from there.
 * One 256-thread workgroup per sequence for the filter (LDS as above), one wave per (sequence, 64 realisations) for the draws: no LDS,
 * no atomics, no barrier.  A call repeats its own bits.
 * GBP_ERR_INVALID_ARG, before any launch: L < 0, n < 1 or n > 1024, n_draws < 1 or > 65536, total_n < L, sizes out of range
 * (total_n * n * n doubles, n_draws * total_n int32), a NULL ptr / n_used / score / g / d2 / filtered / scale / draw_state.  L == 0
 * launches nothing. */
gbp_status gbp_section_draw(int L, const int64_t *ptr, int64_t total_n, int n, const int32_t *n_used, const double *score,
                            const double *g, const double *d2, const int64_t *row_key, uint64_t seed, int n_draws, double *filtered,
                            double *scale, int32_t *draw_state, void *stream);

/* The evidence of the lateral coupling along lines (csrc/gbp_section_evidence.h k_section_evidence; the rule is
 * stated in numpy as sections.evidence_reference): log Z of the chain of gbp_section_track and its derivative in lambda = ln c for a
 * ladder of T scales c_t = 2^t, t = 0 .. T - 1, of the step costs, from one forward pass over d2.  L, ptr, total_n, n, n_used, score,
 * g, d2 as gbp_section_track takes them; g is already multiplied by the lowest scale.
 *   Per sequence and rung t the normalised filter a_t and its tangent b_t = d a_t / d lambda.  Start: a = w_0 / sum w_0, b = 0,
 *   log Z = ln sum w_0 (w = exp(score)), dlog Z = 0.  Per step: cost_0 = g[r] * d2[r, i, j] and e_0 = exp(-cost_0), one multiply and
 *   one exp per entry; e_t = e_{t-1} * e_{t-1} and cost_t = cost_{t-1} + cost_{t-1}; u_j = w_j sum_i a_t[i] e_t[i, j]; u'_j = w_j
 *   sum_i (b_t[i] - a_t[i] cost_t[i, j]) e_t[i, j]; z = sum_j u_j, z' = sum_j u'_j; log Z += ln z, dlog Z += z' / z; a_t = u / z,
 *   b_t = u' / z - a_t (z' / z).  log_partition and dlog_partition f64 [T, L], entry t * L + l.  dlog Z = -E[sum c_t g D^2], the
 *   expected total cost of a section under rung t.  A sequence of one row gives ln sum w_0 and 0.0.  Where a step's z underflows to 0
 *   the rung is -inf or NaN from there on; lower rungs are not affected.  The order of the sums over i and j is the device's own: the
 *   outputs agree with the rule within rounding, not in bits; a call repeats its own bits.
 * One 256-thread workgroup per sequence; no workspace, no atomics.  LDS: the pairs (a_t, b_t) twice, 4 T n doubles, 8 T partial sums
 * and for n <= 128 another 512 T doubles where the lane groups meet: 64.5 KiB at most.
 * GBP_ERR_INVALID_ARG, before any launch: what gbp_section_track refuses of the arguments they share, T < 1 or T > 8, T * n > 2048,
 * a NULL log_partition or dlog_partition.  L == 0 launches nothing. */
gbp_status gbp_section_evidence(int L, const int64_t *ptr, int64_t total_n, int n, const int32_t *n_used, const double *score,
                                const double *g, const double *d2, int T, double *log_partition, double *dlog_partition, void *stream);

/* The terms of the Bethe evidence of the survey graph from the messages of gbp_section_propagate (csrc/gbp_section_evidence.h
 * k_graph_evidence; the rule is stated in numpy as sections.graph_terms_reference).  S, E, n, eu, ev, n_used, g, d2,
 * in_ptr, in_edge as gbp_section_propagate takes them; w f64 [S, n] is its w and message f64 [2 E, n] the half (sweeps & 1) of its mu.
 *   Per edge e = {u, v}: h_u = w_u times the messages into u but v's, h_v likewise (ascending neighbour); K = exp(-(g[e] * d2[e]));
 *   edge_log_z[e] = ln sum_ij h_u[i] K_ij h_v[j]; edge_energy[e] = g[e] sum_ij h_u[i] K_ij d2_ij h_v[j] / that sum: the expected
 *   cost of the edge under its belief.  Per sounding s: node_log_z[s] = ln sum_i w_s[i] times all its incoming messages.
 *   The Bethe evidence is log Z_B = sum_s (1 - deg_s) node_log_z[s] + sum_e edge_log_z[e] -- it does not depend on how the messages
 *   are normalised -- and its derivative in lambda = ln c, c a scale of every g, is -sum_e edge_energy[e]; both sums are the
 *   caller's.  Exact on a forest once the messages have converged; on loops an approximation, as the beliefs are.
 * One launch: a 256-thread workgroup per edge and one per sounding; d2 is read once; no atomics: a call repeats its bits.  The order
 * of the sums is the device's own.  An edge whose endpoints do not fit 0 .. S - 1 gets 0.0 and 0.0.
 * GBP_ERR_INVALID_ARG, before any launch: S < 0, E outside 0 .. 2^30 - 1, n < 1 or n > 256, E > 0 with S < 2, sizes out of range, a
 * NULL n_used / w / in_ptr / node_log_z with S > 0, a NULL eu / ev / g / d2 / in_edge / message / edge_log_z / edge_energy with E > 0.
 * S == 0 launches nothing. */
gbp_status gbp_section_graph_evidence(int S, int E, int n, const int32_t *eu, const int32_t *ev, const int32_t *n_used, const double *w,
                                      const double *g, const double *d2, const int32_t *in_ptr, const int32_t *in_edge,
                                      const double *message, double *node_log_z, double *edge_log_z, double *edge_energy, void *stream);

/* Sections across lines: synchronous sum-product message passing (loopy belief propagation) on a graph of soundings
 * (csrc/gbp_section_graph.h k_graph_kernel, k_graph_init, k_graph_sweep, k_graph_residual, k_graph_belief; the rule is
 * stated in numpy as sections.propagate_reference).  The conventions of gbp_section_track: DEVICE arrays throughout, none read on
 * the host.  S soundings with m_s = n_used[s] (1 .. n) of n <= 256 states and weights w_s = exp(score[s]), score f64 [S, n]; E
 * undirected edges eu[e] < ev[e] int32 [E], sorted by (eu, ev) without duplicates, with g f64 [E] and d2 f64 [E, n, n], [e, i, j]
 * between state i of eu[e] and state j of ev[e]; nothing outside the prefixes i < m_u, j < m_v is read.  Directed edge 2 e is
 * eu -> ev, 2 e + 1 is ev -> eu; in_ptr int32 [S + 1] and in_edge int32 [2 E] are the CSR of every sounding's incoming directed
 * edges, sorted by the sounding they come from.
 *   K_e = exp(-(g[e] * d2[e])).  Messages start at 1 / m_dst.  A sweep computes every message from the last sweep's: for a -> b,
 *   h[i] = w_a[i] times the messages into a from all neighbours but b, ascending neighbour; u[j] = sum_i h[i] K[i, j], i ascending,
 *   one multiply and one add per term; tot = sum_j u[j], j ascending; mu' = u / tot; with damping != 0 mu' = (1 - damping) mu' +
 *   damping mu_old.  residual f64 [sweeps]: the largest |mu' - mu_old| of the sweep (NaN if a message is NaN; 0.0 without edges).
 *   belief f64 [S, n] = w_s times all incoming messages, divided by its sum (i ascending); 0.0 for the states >= m_s.  state int32
 *   [S]: the first maximum of the belief.  A zero tot gives NaN, and the NaN travels as the arithmetic takes it.
 *   The device's exp is not numpy's to the last bit; every other operation is the rule's: a few ulp.  A call repeats its own bits.
 * Workspaces the caller provides: K f64 [E, n, n] (K == d2 works in place), w f64 [S, n], mu f64 [2, 2 E, n], resid f64 [sweeps,
 * 2 E].  One 256-thread workgroup per undirected edge and sweep (35 KiB of static LDS for n <= 64, 41 KiB above), one per sounding for
 * the beliefs.
 * GBP_ERR_INVALID_ARG, before any launch: S < 0, E < 0 or > 2^30 - 1, n < 1 or n > 256, sweeps < 1, damping outside [0, 1), E > 0
 * with S < 2, sizes out of range, a NULL residual, with S > 0 a NULL n_used / score / in_ptr / w / belief / state, with E > 0 a NULL
 * eu / ev / g / d2 / in_edge / K / mu / resid.  An endpoint outside 0 .. S - 1 or an entry of in_edge outside 0 .. 2 E - 1 is
 * skipped on the device, never followed. */
gbp_status gbp_section_propagate(int S, int E, int n, const int32_t *eu, const int32_t *ev, const int32_t *n_used, const double *score,
                                 const double *g, const double *d2, const int32_t *in_ptr, const int32_t *in_edge, int sweeps,
                                 double damping, double *K, double *w, double *mu, double *resid, double *belief, int32_t *state,
                                 double *residual, void *stream);

/* Joint draws of the whole graph of gbp_section_propagate by Gibbs sampling blocked by flight line (csrc/gbp_section_graph_draw.h
 * k_graph_weights, k_graph_line_filter, k_graph_line_draw; the rule is stated in numpy as
 * sections.graph_draw_reference).  DEVICE arrays throughout, none read on the host.  S, E, n, eu, ev, n_used, score, g, d2 as above.
 * ptr int64 [L + 1]: the sequences (flight lines) in the same numbering, contiguous, possibly empty.  An edge with ev = eu + 1 inside
 * one sequence is a step and every consecutive pair of a sequence is one; every other edge joins two sequences: a cross edge.
 *   step_edge int32 [S]: the edge of the step s -> s + 1, -1 at a sequence's last sounding.
 *   cross_ptr int32 [S + 1], cross_edge int32 [cross_ptr[S]]: the CSR of every sounding's incoming CROSS directed edges, ids 2 e
 *   (eu -> ev) and 2 e + 1 (ev -> eu), sorted by the sounding they come from.
 *   colour_ptr int32 [n_colours + 1], colour_line int32 [L]: the sequences grouped by colour; sequences of one colour share no
 *   cross edge (sections.line_colours).
 *   K f64 [E, n, n] = exp(-(g[e] * d2[e])) on the prefixes: with kernel_ready != 0 it already holds what gbp_section_propagate leaves
 *   in its K for the same arguments, and g and d2 are not read (they may be NULL); otherwise the entry fills it first.
 * Sweeps first_sweep .. last_sweep inclusive are run for the realisations rho = first_draw .. first_draw + n_draws - 1, which are
 * independent chains.  Sweep 0, the start, draws every sequence alone, as gbp_section_draw does (cross edges ignored); first_sweep > 0
 * continues from the states in draw_state.  Sweep t >= 1 takes the colours in ascending order and draws every sequence of a colour
 * from its conditional given the other colours' current states by forward filtering and backward sampling, with the weights
 * w'_s[i] = w_s[i] times K_e[i, x_q] (s = eu[e]) or K_e[x_q, i] (s = ev[e]) over the cross edges of s, ascending neighbour q, x_q the
 * neighbour's state; the filter and the walk are those of gbp_section_draw with K read in place of exp(-(g d2)).
 * u = u53(x, y) of Philox4x32-10 with key seed and counter (rho, key & 0xFFFFFFFF, key >> 32, sweep), key = row_key[s] (int64 [S];
 * NULL: s): a draw depends on the seed, the realisation, the sounding's key and the sweep -- not on n_draws, nor on how realisations
 * are cut into calls by first_draw.
 * Outputs: draw_state int32 [n_draws, S] (read when first_sweep > 0; every state < m_s); filtered f64 [n_draws, S, n], the alpha of
 * the last sweep run, 0.0 for the states >= m_s; workspaces w f64 [S, n] and scale f64 [n_draws, S].
 * One 256-thread workgroup per (sequence, realisation) for the filter (LDS: (2 n + 4) doubles), one wave per (sequence, 64
 * realisations) for the walk; no atomics: a call repeats its own bits.
 * GBP_ERR_INVALID_ARG, before any launch: S < 0, E < 0 or > 2^30 - 1, n < 1 or n > 256, L < 0, n_draws < 1 or > 65536, first_draw < 0
 * or first_draw + n_draws > 65536, first_sweep < 0, last_sweep < first_sweep or > 65535, E > 0 with S < 2, S > 0 with L < 1,
 * n_colours outside 1 .. L, sizes out of range, with S > 0 a NULL ptr / n_used / score / step_edge / cross_ptr / colour_ptr /
 * colour_line or a NULL w / filtered / scale / draw_state, with E > 0 a NULL eu / ev / K / cross_edge, and without kernel_ready a NULL
 * g / d2.  S == 0 launches nothing.  An index that does not fit is skipped on the device, never followed. */
gbp_status gbp_section_graph_draw(int S, int E, int n, int L, const int64_t *ptr, const int32_t *eu, const int32_t *ev,
                                  const int32_t *n_used, const double *score, const double *g, const double *d2, int kernel_ready,
                                  double *K, const int32_t *step_edge, const int32_t *cross_ptr, const int32_t *cross_edge,
                                  int n_colours, const int32_t *colour_ptr, const int32_t *colour_line, const int64_t *row_key,
                                  uint64_t seed, int n_draws, int first_draw, int first_sweep, int last_sweep, double *w,
                                  double *filtered, double *scale, int32_t *draw_state, void *stream);

/* The most probable section of the graph of gbp_section_propagate: synchronous max-sum message passing, max-marginals and a decode
 * by conditioning level by level (csrc/gbp_section_graph_path.h k_graph_maxsum, k_graph_maxmarginal, k_graph_condition; DESIGN.md
 * 3.32; the rule is stated in numpy as sections.graph_path_reference).  S, E, n, eu, ev, n_used, score, g, d2, in_ptr, in_edge, sweeps
 * and damping as there: DEVICE arrays, none read on the host.  Everything is in the log domain: theta_s = score[s], c_e[i, j] =
 * g[e] * d2[e, i, j] (one multiply), a message nu[d] has m_dst entries and starts at 0.0.
 *   A sweep computes every message from the last sweep's: for a -> b, h[i] = theta_a[i] plus the messages into a from all neighbours
 *   but b, ascending neighbour; u[j] = the maximum over i < m_a of h[i] - c[i, j], from -inf and replaced on strict > (a NaN candidate
 *   never wins); top = the maximum of u by the same loop; nu' = u - top; with damping != 0 nu' = (1 - damping) nu' + damping nu_old.
 *   A message without a candidate above -inf is NaN.  residual f64 [sweeps]: the largest |nu' - nu_old| of the sweep (NaN if a
 *   message is NaN; 0.0 without edges).
 *   max_marginal f64 [S, n] = theta_s plus all incoming messages (ascending neighbour), minus its maximum; -inf for the states >= m_s.
 *   level int32 [S]: the breadth-first level of every sounding; level_node int32 [S]: the soundings sorted by level; level_ptr int32
 *   [n_levels + 1], a HOST array: the levels' ranges of level_node (sections.decode_levels).  The levels are decided in ascending
 *   order, one launch each: decoded_state[s] = the first maximum over i < m_s of theta_s[i] plus, per neighbour q ascending,
 *   -c at (x_q, i) if level[q] < level[s], else nu[q -> s][i].
 * There is no exp and no reordered sum: the outputs have the rule's bits, and a call repeats them.
 * Workspaces the caller provides: nu f64 [2, 2 E, n] (it leaves the last sweep's messages in half sweeps & 1) and resid f64 [sweeps,
 * 2 E].  One 256-thread workgroup per undirected edge and sweep (37 KiB of static LDS for n <= 64, 43 KiB above), one per sounding for
 * the max-marginals and for the decode.
 * GBP_ERR_INVALID_ARG, before any launch: S < 0, E < 0 or > 2^30 - 1, n < 1 or n > 256, sweeps < 1, damping outside [0, 1), E > 0
 * with S < 2, sizes out of range (S + 2 E, E * n * n, sweeps * 2 E), with S > 0 n_levels outside 1 .. S, a NULL n_used / score /
 * in_ptr / level_ptr / level_node / level / max_marginal / decoded_state / residual or a level_ptr that does not start at 0, end at S
 * or that decreases, with E > 0 a NULL eu / ev / g / d2 / in_edge / nu / resid.  S == 0 launches nothing.  An index that does not
 * fit is skipped on the device, never followed; a neighbour's state is clamped into its prefix. */
gbp_status gbp_section_graph_path(int S, int E, int n, const int32_t *eu, const int32_t *ev, const int32_t *n_used, const double *score,
                                  const double *g, const double *d2, const int32_t *in_ptr, const int32_t *in_edge, int sweeps,
                                  double damping, int n_levels, const int32_t *level_ptr, const int32_t *level_node,
                                  const int32_t *level, double *nu, double *resid, double *max_marginal, int32_t *decoded_state,
                                  double *residual, void *stream);

/* Coordinate ascent on the exact score sum_s score[s, x_s] - sum_e g[e] d2[e, x_u, x_v] of C sections of the same graph
 * (csrc/gbp_section_graph_path.h k_graph_condition; sections.refine_reference states the rule).  state int32 [C, S]
 * holds the sections (every state < m_s) and is replaced in place.  colour_node int32 [S]: the soundings sorted by colour, soundings
 * of one colour sharing no edge; colour_ptr int32 [n_colours + 1], a HOST array: the colours' ranges (sections.sounding_colours).
 * A sweep takes the colours in ascending order, one launch each, the soundings of a colour together: v[i] = theta_s[i] minus, per
 * neighbour q ascending, c at (x_q, i); the sounding moves to the first maximum of v over i < m_s only if v there is strictly greater
 * than v at its state, so every move raises the score.  moves int32 [C, refine]: the moves of every section in every sweep, counted
 * by one integer atomic per workgroup (exact in any order); all `refine` sweeps are launched, and a section that has stopped moving
 * counts 0 from then on.  A call repeats its bits.
 * GBP_ERR_INVALID_ARG, before any launch: S < 0, E < 0 or > 2^30 - 1, n < 1 or n > 256, C outside 1 .. 65537, refine outside
 * 0 .. 65536, E > 0 with S < 2, sizes out of range (S + 2 E, E * n * n, C * S), with S > 0 n_colours outside 1 .. S, a NULL n_used /
 * score / in_ptr / colour_ptr / colour_node / state, a NULL moves with refine > 0, or a colour_ptr that does not start at 0, end at S
 * or that decreases, with E > 0 a NULL eu / ev / g / d2 / in_edge.  S == 0 or refine == 0 launches nothing. */
gbp_status gbp_section_graph_refine(int S, int E, int n, int C, const int32_t *eu, const int32_t *ev, const int32_t *n_used,
                                    const double *score, const double *g, const double *d2, const int32_t *in_ptr,
                                    const int32_t *in_edge, int n_colours, const int32_t *colour_ptr, const int32_t *colour_node,
                                    int refine, int32_t *state, int32_t *moves, void *stream);

/* Horizons across lines: the graph of gbp_section_propagate with the states and the pair term of gbp_horizon_track
 * (csrc/gbp_horizon_graph.h k_hgraph_init, k_hgraph_sweep, k_hgraph_node, k_hgraph_condition; the rules are stated in
 * numpy as horizons.propagate_reference, horizons.graph_path_reference and horizons.refine_reference).  DEVICE arrays throughout, none
 * read on the host but level_ptr / colour_ptr, which are HOST arrays.  N soundings share S cells of width dz (1 .. 2048) and, with
 * has_absent = 1, the absent state S: SA = S + has_absent states; score f64 [N, SA], the absent state's score last.  E undirected edges
 * eu[e] < ev[e] int32 [E], sorted by (eu, ev) without duplicates, with g f64 [E] and d f64 [E] (horizons.graph_steps); cell a under
 * eu[e] and cell b under ev[e] cost T_e[b - a] = g[e] * fabs(d[e] - (double)(b - a) * dz); cell <-> absent costs switch_cost >= 0,
 * absent <-> absent 0.  Directed edge 2 e is eu -> ev, 2 e + 1 is ev -> eu; in_ptr int32 [N + 1] and in_edge int32 [2 E] are the CSR of
 * every sounding's incoming directed edges, sorted by the sounding they come from (sections.incoming).  A message's source states are
 * visited cells ascending, then absent.
 *   gbp_horizon_graph_propagate: sum-product.  w = exp(score), K_e = exp(-T_e), ks = exp(-switch_cost); messages start at 1 / SA; for
 *   a -> b, h = w_a times the messages into a from all neighbours but b (ascending neighbour); u[j] = sum_i h[i] K (cells i ascending)
 *   + h[S] ks for a cell j, u[S] = sum_i h[i] ks + h[S]; tot = sum_j u[j], j ascending, by one lane; mu' = u / tot; with damping != 0
 *   mu' = (1 - damping) mu' + damping mu_old.  residual f64 [sweeps]: the largest |mu' - mu_old| of the sweep (NaN if a message is;
 *   0.0 without edges).  belief f64 [N, SA] = w_s times all incoming messages, divided by its sum (ascending); state int32 [N]: its
 *   first maximum.  A zero tot gives NaN.  The device's exp is not numpy's to the last bit; every other operation is the rule's.
 *   Workspaces: w f64 [N, SA], mu f64 [2, 2 E, SA], resid f64 [sweeps, 2 E].
 *   gbp_horizon_graph_path: max-sum in the log domain, no exp.  Messages start at 0.0; u[j] = the maximum of h[i] - T (cells i
 *   ascending, from -inf on strict >), then h[S] - switch_cost; u[S] of h[i] - switch_cost, then h[S]; nu' = u minus its first maximum;
 *   damping and residual as above.  max_marginal f64 [N, SA] = score_s plus all incoming messages, minus its maximum.  level,
 *   level_node, level_ptr as gbp_section_graph_path takes them (sections.decode_levels): decoded_state[s] = the first maximum of
 *   score_s[i] minus, per neighbour q ascending, the pair cost at x_q if level[q] < level[s], else plus nu[q -> s][i].  The outputs have
 *   the rule's bits.  Workspaces: nu f64 [2, 2 E, SA] (the last sweep's messages are left in half sweeps & 1), resid f64 [sweeps, 2 E].
 *   gbp_horizon_graph_refine: coordinate ascent of C horizons state int32 [C, N] in place, as gbp_section_graph_refine: colour_node,
 *   colour_ptr of sections.sounding_colours; a sounding moves to the first maximum of v[i] = score_s[i] minus the pair costs at its
 *   neighbours' states only if v there is strictly greater than at its state; moves int32 [C, refine].
 * One 256-thread workgroup per undirected edge and sweep with (4 S + 2) doubles of dynamic LDS (65 552 B at S = 2048), one per sounding
 * for the beliefs, the max-marginals, the decode and the ascent.  No float atomics: a call repeats its bits.
 * GBP_ERR_INVALID_ARG, before any launch and naming the entry: N < 0, E < 0 or > 2^30 - 1, S < 1 or > 2048, has_absent not 0 or 1, dz
 * not positive, switch_cost negative or not finite, E > 0 with N < 2, sizes out of range (N + 2 E, N * SA, 2 * 2 E * SA, sweeps * 2 E,
 * C * N), sweeps < 1, damping outside [0, 1), C outside 1 .. 65537, refine outside 0 .. 65536, with N > 0 n_levels / n_colours outside
 * 1 .. N, a NULL score / in_ptr / output / group array or a group_ptr that does not start at 0, end at N or that decreases, with E > 0 a
 * NULL eu / ev / g / d / in_edge / message or resid workspace.  N == 0 launches nothing that reads a sounding, E == 0 nothing that reads
 * an edge.  An index that does not fit is skipped on the device, never followed; a neighbour's state is clamped into 0 .. SA - 1. */
gbp_status gbp_horizon_graph_propagate(int N, int E, int S, int has_absent, double dz, double switch_cost, const int32_t *eu,
                                       const int32_t *ev, const double *score, const double *g, const double *d, const int32_t *in_ptr,
                                       const int32_t *in_edge, int sweeps, double damping, double *w, double *mu, double *resid,
                                       double *belief, int32_t *state, double *residual, void *stream);
gbp_status gbp_horizon_graph_path(int N, int E, int S, int has_absent, double dz, double switch_cost, const int32_t *eu,
                                  const int32_t *ev, const double *score, const double *g, const double *d, const int32_t *in_ptr,
                                  const int32_t *in_edge, int sweeps, double damping, int n_levels, const int32_t *level_ptr,
                                  const int32_t *level_node, const int32_t *level, double *nu, double *resid, double *max_marginal,
                                  int32_t *decoded_state, double *residual, void *stream);
gbp_status gbp_horizon_graph_refine(int N, int E, int S, int has_absent, double dz, double switch_cost, int C, const int32_t *eu,
                                    const int32_t *ev, const double *score, const double *g, const double *d, const int32_t *in_ptr,
                                    const int32_t *in_edge, int n_colours, const int32_t *colour_ptr, const int32_t *colour_node,
                                    int refine, int32_t *state, int32_t *moves, void *stream);

/* Joint draws of horizons along lines from the chain of gbp_horizon_track by forward filtering and backward sampling
 * (csrc/gbp_horizon_draw.h k_horizon_filter, k_horizon_walk; the rule is stated in numpy as horizons.draw_reference).
 * L, ptr, total_n, max_n, S, dz, score, absent_score (NULL: no absent state), g, d, switch_cost as gbp_horizon_track takes them, with
 * one difference: a sequence may be empty (ptr repeated; nothing is written for it).  n_states = S + 1 with absent_score, else S.
 *   Filter: the forward half of the marginals of gbp_horizon_track, operation for operation: filtered f64 [total_n, n_states] =
 *   alpha_n (the absent state last), scale [total_n] = s_n.
 *   Walk: realisation rho = 0 .. n_draws - 1 walks n = last .. first of every sequence over the states i = 0 .. n_states - 1, cells
 *   ascending and absent last; j is the state just drawn under n + 1.  W[i] = alpha_n[i] at the sequence's last row; elsewhere
 *   alpha_n[i] * K_n[j - i] for cells i and j, alpha_n[i] * ks for a cell i and j absent, alpha_n[S] * ks for i absent and a cell j,
 *   alpha_n[S] (no multiply) for both absent.  c[i] = c[i - 1] + W[i], i ascending; thr = u * c[n_states - 1]; the state is
 *   min(#{i : c[i] <= thr}, n_states - 1): a state of weight 0 is never drawn, and with a NaN total the state is 0.  u = u53(x, y) of
 *   Philox4x32-10 with key seed and counter (rho, key & 0xFFFFFFFF, key >> 32, 0), key = row_key[n] (int64 [total_n]; NULL: n): the
 *   counter layout of gbp_section_draw.  A draw depends on the seed, the realisation and the row's key, not on n_draws nor on how
 *   sequences are grouped into launches.  draw_state int32 [n_draws, total_n], S meaning absent.  The device's exp is not numpy's to
 *   the last bit: a draw whose threshold lies within rounding of a c[i] may fall either way, and the walk differs from there.
 * One 256-thread workgroup per sequence for the filter, LDS (4 S + 6) doubles; one 256-thread workgroup per (sequence, 256
 * realisations) for the walk, lane = realisation, LDS (3 S + 1) doubles.  No atomics: a call repeats its bits.
 * GBP_ERR_INVALID_ARG, before any launch: L < 0, S < 1 or S > 2048, n_draws < 1 or > 65536, dz not positive, switch_cost negative or
 * not finite, total_n < 0, max_n > total_n, L * max_n < total_n, total_n * (S + 1) or n_draws * total_n out of range, a NULL ptr /
 * score / g / d / filtered / scale / draw_state.  L == 0 or total_n == 0 launches nothing. */
gbp_status gbp_horizon_draw(int L, const int64_t *ptr, int64_t total_n, int max_n, int S, double dz, const double *score,
                            const double *absent_score, const double *g, const double *d, double switch_cost, const int64_t *row_key,
                            uint64_t seed, int n_draws, double *filtered, double *scale, int32_t *draw_state, void *stream);

/* Joint draws of horizons across lines: Gibbs sampling blocked by flight line on the graph of gbp_horizon_graph_propagate
 * (csrc/gbp_horizon_draw.h k_horizon_filter<NJ, true>, k_horizon_walk<false>; the rule is stated in numpy as
 * horizons.graph_draw_reference).  N, E, S, has_absent, dz, switch_cost, eu, ev, score [N, SA] (the absent state's column last), g,
 * d [E] as gbp_horizon_graph_propagate takes them; L, ptr [L + 1] int64: the sequences (lines) in the same numbering, contiguous,
 * possibly empty; step_edge int32 [N]: the edge of the step n -> n + 1 inside a sequence, -1 at its last sounding; cross_ptr
 * [N + 1], cross_edge: the CSR of every sounding's incoming cross edges, ids 2 e (from eu[e]) and 2 e + 1 (from ev[e]), neighbours
 * ascending; colour_ptr [n_colours + 1], colour_line [L]: the sequences grouped by colour, sequences of one colour sharing no edge.
 *   Sweep 0 (only when first_sweep == 0): every sequence alone, gbp_horizon_draw's filter and walk with the step edges' (g, d).
 *   Sweep t = max(first_sweep, 1) .. sweeps: colours ascending; for every sequence of the colour and realisation the same filter and
 *   walk with w' in place of w: w'_s[i] = w_s[i] times, per cross edge of s in CSR order, exp(-(g_e * fabs(d_e - k * dz))) between
 *   cells with k = x_q - i for s = eu[e] and i - x_q for s = ev[e], x_q the neighbour's current state (clamped into 0 .. SA - 1);
 *   exp(-switch_cost) between a cell and absent; nothing between absent and absent.  States are replaced in place.
 *   u = u53(x, y) of Philox4x32-10 with key seed and counter (first_draw + r, key & 0xFFFFFFFF, key >> 32, t), r the realisation
 *   within the call, key = row_key[n] (NULL: n): cutting realisations into calls changes no draw.
 * alpha f64 [n_draws, N, SA] (the filtered rows of the last sweep in which each sounding was drawn; after sweep 0 alone only slab 0 is
 * written, shared by all realisations), scale f64 [n_draws, N], draw_state int32 [n_draws, N] (read when first_sweep > 0).
 * An index that does not fit (edge, sounding, sequence, colour) is skipped, never followed.  No atomics: a call repeats its bits.
 * GBP_ERR_INVALID_ARG, before any launch: the refusals of gbp_horizon_graph_propagate on N, E, S, has_absent, dz, switch_cost; L < 0,
 * or L < 1 with N > 0; n_draws outside 1 .. 65536; first_draw + n_draws beyond 65536; sweeps outside first_sweep .. 65535; n_colours
 * outside 1 .. L (the colour lists must cover the sequences); n_draws * N * SA, n_draws * N or L * n_draws out of range; NULL
 * pointers (row_key may be NULL; eu, ev, g, d, cross_edge only with E > 0).  N == 0 launches nothing. */
gbp_status gbp_horizon_graph_draw(int N, int E, int S, int has_absent, double dz, double switch_cost, const int32_t *eu,
                                  const int32_t *ev, const double *score, const double *g, const double *d, int L, const int64_t *ptr,
                                  const int32_t *step_edge, const int32_t *cross_ptr, const int32_t *cross_edge, int n_colours,
                                  const int32_t *colour_ptr, const int32_t *colour_line, const int64_t *row_key, uint64_t seed,
                                  int n_draws, int first_draw, int first_sweep, int sweeps, double *alpha, double *scale,
                                  int32_t *draw_state, void *stream);

/* Connected bodies of R realisations of a raster (csrc/gbp_bodies.h k_bodies_label; the rule is stated in numpy as
 * bodies.label_reference).  raster f64 [R, S, C]: S soundings, C cells each (depth or ONE elevation axis).  A cell is a member iff
 * lo <= v <= hi in fp64 (a NaN never is; +-inf bounds give one-sided thresholds).  Cells (s, c) and (s, c + 1) are adjacent, and
 * (eu[e], c) and (ev[e], c) for every edge e of eu / ev int32 [E]: undirected, in either direction, repeats allowed.  A body is a
 * connected set of members.  group_ptr int64 [G + 1] cuts the soundings into contiguous ranges (possibly empty) that no edge leaves;
 * the edges come group by group: the group of eu[e] does not decrease along e.  DEVICE arrays throughout; group_ptr, eu and ev are
 * also copied to the host and checked before the launch, which waits for the stream's earlier work (the one departure from
 * gbp_section_graph_draw: an edge that does not fit would be followed outside the outputs).
 * Outputs, per realisation: label int32 [R, S, C], -1 for a non-member, else the smallest s * C + c of the cell's body; cells int32
 * [R, S, C], the number of cells of the body at its root (the cell whose index is its label), 0 elsewhere; measure_q int64 [R, S, C],
 * at the root the sum over the body of q(s, c) = rint((a[s] * t[c]) / unit), one IEEE operation each, 0 elsewhere, a f64 [S] and t
 * f64 [C] finite and >= 0 (the caller's to check) with q <= 2^30 when unit = (max a * max t) * 2^-30.  a and t may both be NULL: then
 * measure_q is not written and may be NULL.  sweeps int32 [R, G]: the sweeps of lateral merging the workgroup took (0 for a group
 * without edges or soundings).  Integer outputs: exact, independent of any order, and a call repeats its bits.
 * One 1024-thread workgroup per (realisation, group); 4 B of static LDS; no workgroup reads a word another one writes.
 * GBP_ERR_INVALID_ARG, before any launch: R outside 1 .. 65536, S < 0, C outside 1 .. 4096, E outside 0 .. 2^30 - 1, G outside
 * 0 .. S, R * S * C >= 2^31, R * G out of range, E > 0 with S < 1, S > 0 with G < 1, one of a / t alone, with a and t a unit that is
 * not finite and > 0, with S > 0 a NULL group_ptr / raster / label / cells / sweeps (or measure_q with a and t), with E > 0 a NULL
 * eu / ev, a group_ptr that does not start at 0, end at S or that decreases, an edge's sounding outside 0 .. S - 1, edges not sorted
 * by the group of eu, an edge that joins two groups.  S == 0 launches nothing. */
gbp_status gbp_bodies_label(int R, int S, int C, int E, int G, const int64_t *group_ptr, const int32_t *eu, const int32_t *ev,
                            const double *raster, double lo, double hi, const double *a, const double *t, double unit, int32_t *label,
                            int32_t *cells, int64_t *measure_q, int32_t *sweeps, void *stream);

/* Borehole logs as a log weight of the kept models (csrc/gbp_boreholes.h k_borehole_score; the rule is stated in numpy
 * as boreholes.score_reference).  The ensemble and rows int32 [S, n] / n_used int32 [S] are those of gbp_ensemble_cross_distance; model
 * m of sounding s is rows[s, m], absent when m >= n_used[s], the row lies outside the slots or k <= 0.  Nb boreholes hold I intervals
 * (bore_ptr int32 [Nb + 1]): top, bottom f64 [I] in metres below the collar, ascending and not overlapping within a borehole; cls int32
 * [I] is -1 for a MEASURED interval (value f64 log10 S/m, sd f64 > 0 decades) and a class in 0 .. C - 1 for a LITHOLOGY interval.
 * The A attachments of borehole att_bore[a] to sounding s are att_ptr[s] .. att_ptr[s + 1] - 1 (int32 [S + 1]), each with att_var >= 0
 * (decades^2) and att_shift (m).  DEVICE arrays throughout but class_mean, class_scale, class_ln_prior (HOST, f64 [C]).
 * For every attachment a of s in order, every interval in order and every present model with interfaces e and a_l = log10 sigma_l:
 * t' = max(top + shift, 0), b' = bottom + shift; b' <= t' is skipped and counted in skipped[a]; h = b' - t'; the segments [p, q] are
 * the merge of [t', b'] with the layers, from the layer after the last interface <= t', q = fmin(next interface, b'), the layer
 * advanced where the interface == q; mean = (sum (q - p) f_l) / h.  MEASURED: f_l = a_l, term = -((mean - value)^2) / (2 (sd^2 + var)).
 * LITHOLOGY of class c: l_q(x) = ln_prior_q - 0.5 ln(v_q) - (x - mean_q)^2 / (2 v_q), v_q = scale_q^2 + var; f_l = 1 / sum_q
 * exp(l_q(a_l) - l_c(a_l)), q ascending; term = ln(class_floor + (1 - class_floor) mean).  part[a, m] = the sum of the terms,
 * score[s, m] = the sum of the parts in attachment order; 0.0 for an absent model and for a sounding without attachments.  Constants
 * common to all models of a sounding are dropped; the interval mean is taken in log10 conductivity.
 * Outputs: score f64 [S, n], every entry written; part f64 [A, n] and skipped int32 [A], each of which may be NULL.
 * One wave per (sounding, 64 models); dynamic LDS 64 (2 K - 1) doubles; no atomics: a call repeats its bits.  att_ptr, att_bore,
 * bore_ptr and cls are copied to the host and checked before the launch, which waits for the stream's earlier work.
 * GBP_ERR_INVALID_ARG, before any launch: S < 0, n_slots < 1, n outside 1 .. 1024, K outside 1 .. 64, C outside 0 .. 16, A, Nb or I
 * < 0, A > 0 with Nb < 1, class_floor outside (0, 1), with C > 0 a NULL class array, a class mean or log prior that is not finite, a
 * class scale that is not finite and positive, sizes out of range, with S > 0 a NULL ensemble / rows / n_used / att_ptr / score, with
 * A > 0 a NULL att_bore / att_var / att_shift / bore_ptr, with A > 0 and I > 0 a NULL interval array, an att_ptr or bore_ptr that does
 * not start at 0, end at A (I) or that decreases, an attachment's borehole outside 0 .. Nb - 1, a class outside -1 .. C - 1.
 * S == 0 launches nothing. */
gbp_status gbp_borehole_score(int S, int n_slots, int K, const int32_t *ens_k, const double *ens_edges, const double *ens_sigma, int n,
                              const int32_t *rows, const int32_t *n_used, int A, const int32_t *att_ptr, const int32_t *att_bore,
                              const double *att_var, const double *att_shift, int Nb, const int32_t *bore_ptr, int I, const double *top,
                              const double *bottom, const double *value, const double *sd, const int32_t *cls, int C,
                              const double *class_mean, const double *class_scale, const double *class_ln_prior, double class_floor,
                              double *score, double *part, int32_t *skipped, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOBIPY_AMD_H */
