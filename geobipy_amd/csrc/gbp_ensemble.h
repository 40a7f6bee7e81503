// Kernels on a finished posterior ensemble (gbp_rj_chains.ens_k / ens_edges / ens_sigma: the sampled models a chain kept,
// include/geobipy_amd.h states the rule).  Included by gbp_fdem.hip after gbp_rjmcmc.h: the re-binning kernel calls
// the sampler's own accumulators.
//   k_ensemble_raster   realisations on a depth axis: the conductivity of the layer holding every cell centre, a pure gather
//   k_ensemble_rebin    the hit map / unit posteriors of the kept models on axes chosen after the run
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gbp_ensemble_series.h"

namespace ensemble {

// One wave per output row (chain b, list entry r) loads its slot once (gbp_ensemble_series.h states the raster rule; the stored
// doubles, so the output is the stored double bit for bit).  A pass covers CELLS * 64 cells; lane i owns cells c0 + i + 64 j, so every
// store instruction of the wave writes one contiguous 512-byte run.  A slot outside the ensemble or an empty one (k == 0) gives a row
// of NaN.
template <int CELLS>
__global__ __launch_bounds__(256) void k_ensemble_raster(long long rows, int ne, int K, int R, int nz, const int* __restrict__ ens_k,
                                                         const double* __restrict__ ens_edges, const double* __restrict__ ens_sigma,
                                                         const int* __restrict__ slots, const double* __restrict__ z,
                                                         double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long b = row / R;
    const int slot = slots[(int)(row - b * R)];
    const bool inside = slot >= 0 && slot < ne;
    const Slot q = slot_load<false>(ens_k, ens_edges, ens_sigma, K, (size_t)(b * ne + (inside ? slot : 0)), inside, lane);
    double* __restrict__ o = out + row * nz;
    for (int c0 = 0; c0 < nz; c0 += 64 * CELLS) {
        double zc[CELLS], v[CELLS];
#pragma unroll
        for (int j = 0; j < CELLS; ++j) zc[j] = z[min(c0 + lane + 64 * j, nz - 1)];
        layers<CELLS>(q, zc, v);
#pragma unroll
        for (int j = 0; j < CELLS; ++j) {
            const int c = c0 + lane + 64 * j;
            if (c < nz) o[c] = v[j];
        }
    }
}

// One wave per chain walks the filled slots in order and adds every kept model with weight 1 through the sampler's own
// hitmap_add<64> / units_add<64> (csrc/gbp_rjmcmc.h): the same expressions, the same bits as a sampler that had binned on these axes.
// A lane owns its cells / units / thresholds for the whole walk, so plain adds suffice (as in the sampler).  o: the axes, units and
// thresholds; c: B, log_mean_prior, ens_*, and the outputs hitmap (may be NULL), unit_z / unit_hist, first_hist / first_none.
__global__ __launch_bounds__(64) void k_ensemble_rebin(rj::RjOpt o, gbp_rj_chains c)
{
    const size_t b = blockIdx.x;
    const int lane = threadIdx.x, ne = o.n_ensemble, K = o.max_layers;
    const double lmp = c.log_mean_prior[b];
    const size_t nh = (size_t)o.n_value_bins * o.n_depth_bins;
    for (int s = 0; s < ne; ++s) {
        const size_t row = b * ne + s;
        const int k = min(c.ens_k[row], K);
        if (k <= 0) continue;
        if (c.hitmap != nullptr) rj::hitmap_add<64>(o, c.hitmap + b * nh, c.ens_edges + row * K, c.ens_sigma + row * K, k, lmp, lane, 1);
        if (rj::units_on(c)) rj::units_add<64>(o, c, b, c.ens_edges + row * K, c.ens_sigma + row * K, k, lmp, lane, 1);
    }
}

}  // namespace ensemble
