// Posterior correlation between the variables of regularly spaced series (the rule: include/geobipy_amd.h
// gbp_series_correlation and geobipy_amd/ensembles.py correlation_reference): per sounding the band R(c, c + j), j = 0 .. W, of the
// pooled sample correlation (or covariance) matrix of the used rows, and the runs of a band above a threshold.  Included by
// gbp_fdem.hip after gbp_ensemble_diag.h.  SOURCE: the two sources of gbp_ensemble_series.h (RASTER: the log10 conductivity at the
// cell centres, built on the fly; the slot is loaded once per row and serves every staged column).
// Four launches, each a pure function of what the one before wrote -- no workgroup reads what another of its launch writes:
//   k_series_moments<SOURCE>      one workgroup of 4 waves per (sounding, 64 variables): every used row once; stats[b, 0, v] = the mean
//                                 (a constant's value as stored; NaN for a non-finite sample), stats[b, 1, v] = the flag 1 (live),
//                                 0 (constant) or NaN (non-finite, M = 0, n < 4)
//   k_series_correlation<SOURCE>  one workgroup of 4 waves per (sounding, strip of 4 tile rows = 64 variables, panel of 8 tile
//                                 diagonals): chunks of CORR_CH centred rows d = x - mean are staged in LDS -- 0 for rows past the last
//                                 used one, for variables past V and for variables that are not live -- with a row stride S = 16 mod
//                                 32 doubles, so the ds_read_b64 of 16 consecutive doubles from 4 consecutive rows (one MFMA operand)
//                                 touches every bank once per half wave.  Wave w owns tile row I = 4 strip + w: per 4 rows it reads its A
//                                 operand once and walks its tiles J = I + 8 panel + q, q < 8, one v_mfma_f64_16x16x4_f64 and one
//                                 accumulator (4 doubles per lane) each.  A[i][k] = d[t0 + k][16 I + i], B[k][j] = d[t0 + k][16 J + j],
//                                 one f64 per lane, lane = index + 16 k; C/D: col = lane & 15, row = (lane >> 4) + 4 reg.  The finish
//                                 writes sum / (n - 1) to band[b, c, j]: the 16 lanes of a C row hold consecutive j, 128-byte runs.
//                                 W <= 112 is one panel; the full band of 440 cells is four, and the rows are staged once per panel.
//   k_correlation_sd              a lane per (sounding, variable): a live variable's flag becomes sd = sqrt(band[b, v, 0])
//   k_correlation_finish          a lane per band entry: NaN past the axis and where either variable is not live, the diagonal of a
//                                 live variable 1 exactly, the rest divided by sd_u sd_v (normalise) or left as the covariance
//   k_band_runs                   a lane per (sounding, cell): the runs of band entries >= threshold up and down from the cell
// No atomics; every sum has one order, so a call repeats its own bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gbp_ensemble_series.h"

namespace ensemble {

constexpr int CORR_WAVES = 4, CORR_CH = 32, CORR_NACC = 8, CORR_MAX_GROUPS = 4;
constexpr int CORR_MAX_COLS = (CORR_NACC + CORR_WAVES - 1) * 16 + CORR_WAVES * 16;          // 240: a panel's B tiles and, beyond panel 0, the strip's A tiles
constexpr size_t CORR_LDS_BYTES = (size_t)CORR_CH * CORR_MAX_COLS * sizeof(double);        // 61 440 B at most (240 = 16 mod 32: no padding)
static_assert(CORR_MAX_COLS <= 64 * CORR_MAX_GROUPS && CORR_MAX_COLS % 32 == 16, "a staged row is at most four groups of 64 lanes");

typedef double corr_double4 __attribute__((ext_vector_type(4)));

struct CorrArgs : SeriesArgs {           // reach: W
    double* stats;                    // [B, 2, V]: mean; flag, then sd
    double* band;                     // [B, V, W + 1]
};

template <int SOURCE>
__global__ __launch_bounds__(CORR_WAVES * 64) void k_series_moments(CorrArgs a)
{
    __shared__ double red[4][CORR_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int V = a.V, tiles = (V + 63) / 64;
    const size_t b = blockIdx.x / tiles;
    const int v = (int)(blockIdx.x % tiles) * 64 + lane;
    const bool own = v < V;
    const int vc = min(v, V - 1);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const Segments seg = series_segments(a, b);
    const int M = seg.M, N = seg.N;
    double* const st = a.stats + b * 2 * (size_t)V;
    if (M <= 0 || N <= 0 || (int64_t)M * N < 4) {
        if (w == 0 && own) st[v] = st[(size_t)V + v] = qnan;
        return;
    }
    const int* const seg0 = series_starts(a, b);
    const double zc = SOURCE == SERIES_RASTER ? a.z[vc] : 0.0;
    double s = 0.0, lo = (double)INFINITY, hi = -(double)INFINITY;
    int nf = 0;
    for (int m = 0; m < M; ++m) {
        const int r0 = __builtin_amdgcn_readfirstlane(seg0[m]);
        for (int t = w; t < N; t += CORR_WAVES) {
            double x;
            const size_t src = series_row(a, b, r0 + t);
            if (SOURCE == SERIES_PLAIN) x = a.x[src * (size_t)V + vc];
            else layers<1>(slot_load(a, src, lane), &zc, &x);
            s += x;
            lo = fmin(lo, x);
            hi = fmax(hi, x);
            nf |= (__double2hiint(x) & 0x7ff00000) == 0x7ff00000 ? 1 : 0;
        }
    }
    red[0][w][lane] = s;
    red[1][w][lane] = lo;
    red[2][w][lane] = hi;
    red[3][w][lane] = (double)nf;
    __syncthreads();
    if (w != 0 || !own) return;
    double total = 0.0, mn = (double)INFINITY, mx = -(double)INFINITY;
    bool bad = false;
    for (int u = 0; u < CORR_WAVES; ++u) {
        total += red[0][u][lane];
        mn = fmin(mn, red[1][u][lane]);
        mx = fmax(mx, red[2][u][lane]);
        bad |= red[3][u][lane] != 0.0;
    }
    const bool constant = !bad && mn == mx;
    st[v] = bad ? qnan : (constant ? mn : total / (double)(M * N));
    st[(size_t)V + v] = bad ? qnan : (constant ? 0.0 : 1.0);
}

template <int SOURCE>
__global__ __launch_bounds__(CORR_WAVES * 64) void k_series_correlation(CorrArgs a, int npanels)
{
    extern __shared__ __attribute__((aligned(16))) double corr_lds[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int V = a.V, W = a.reach, ntiles = (V + 15) / 16, nstrips = (ntiles + CORR_WAVES - 1) / CORR_WAVES;
    const int DJ = (W + 15) / 16 + 1;                                  // tile diagonals a tile row meets: J - I = 0 .. ceil(W / 16)
    const int panel = (int)(blockIdx.x % npanels);
    const int strip = (int)((blockIdx.x / npanels) % nstrips);
    const size_t b = blockIdx.x / npanels / nstrips;
    const Segments seg = series_segments(a, b);
    const int M = seg.M, N = seg.N;
    if (M <= 0 || N <= 0 || (int64_t)M * N < 4) return;                // (the finish writes NaN: the flags say so)
    const int n = M * N;
    const int Jbase = strip * CORR_WAVES + CORR_NACC * panel;          // the panel's first B tile
    if (Jbase >= ntiles) return;
    const int nb = min(min(DJ - CORR_NACC * panel, CORR_NACC) + CORR_WAVES - 1, ntiles - Jbase);        // its B tiles
    const int a_off = panel == 0 ? 0 : nb * 16;                        // where the strip's own columns are staged
    const int ncol = nb * 16 + (panel == 0 ? 0 : CORR_WAVES * 16);
    const int S = ncol + ((ncol & 31) == 0 ? 16 : 0);                  // S = 16 mod 32
    const int ngroups = (ncol + 63) / 64;
    const double* const st = a.stats + b * 2 * (size_t)V;
    {   // a strip without a live variable has nothing to add (the deep cells of a depth axis)
        const int v = strip * 64 + lane;
        if (__ballot(v < V && st[(size_t)V + min(v, V - 1)] > 0.0) == 0ull) return;
    }
    // what this lane stages: column q = 64 g + lane of the LDS row is variable v[g]
    double mean[CORR_MAX_GROUPS], zc[CORR_MAX_GROUPS];
    int vcol[CORR_MAX_GROUPS];
    bool live[CORR_MAX_GROUPS];
#pragma unroll
    for (int g = 0; g < CORR_MAX_GROUPS; ++g) {
        const int q = 64 * g + lane;
        const int v = q < nb * 16 ? Jbase * 16 + q : strip * 64 + (q - nb * 16);
        const int vc = min(max(v, 0), V - 1);
        vcol[g] = vc;
        live[g] = q < ncol && v < V && st[(size_t)V + vc] > 0.0;
        mean[g] = st[vc];
        zc[g] = SOURCE == SERIES_RASTER ? a.z[vc] : 0.0;
    }
    const int* const seg0 = series_starts(a, b);
    const int I = strip * CORR_WAVES + w;
    const int nq = I < ntiles ? min(min(CORR_NACC, DJ - CORR_NACC * panel), ntiles - (I + CORR_NACC * panel)) : 0;      // this wave's tiles (<= 0: none)
    corr_double4 acc[CORR_NACC];
#pragma unroll
    for (int q = 0; q < CORR_NACC; ++q) acc[q] = corr_double4{0.0, 0.0, 0.0, 0.0};
    const int arow = (lane >> 4) * S + (lane & 15);

    for (int c0 = 0; c0 < n; c0 += CORR_CH) {
        for (int rr = w; rr < CORR_CH; rr += CORR_WAVES) {
            const int r = c0 + rr;
            double x[CORR_MAX_GROUPS] = {0.0, 0.0, 0.0, 0.0};
            if (r < n) {
                const int m = r / N;
                const size_t src = series_row(a, b, __builtin_amdgcn_readfirstlane(seg0[m]) + r - m * N);
                if (SOURCE == SERIES_PLAIN) {
#pragma unroll
                    for (int g = 0; g < CORR_MAX_GROUPS; ++g)
                        if (live[g]) x[g] = a.x[src * (size_t)V + vcol[g]];
                } else {
                    const Slot slot = slot_load(a, src, lane);
                    if (ngroups <= 2) layers<2>(slot, zc, x);          // (the columns past 128 stay 0: not staged)
                    else layers<CORR_MAX_GROUPS>(slot, zc, x);
                }
            }
#pragma unroll
            for (int g = 0; g < CORR_MAX_GROUPS; ++g) {
                const int q = 64 * g + lane;
                if (q < ncol) corr_lds[rr * S + q] = live[g] && r < n ? x[g] - mean[g] : 0.0;
            }
        }
        __syncthreads();
        if (nq > 0) {
            for (int kk = 0; kk < CORR_CH / 4; ++kk) {
                const double* const row = corr_lds + kk * 4 * S + arow;
                const double av = row[a_off + 16 * w];
#pragma unroll
                for (int q = 0; q < CORR_NACC; ++q)
                    if (q < nq) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, row[16 * (w + q)], acc[q], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- finish: C / (n - 1) into the band; lane holds C[row = (lane >> 4) + 4 reg][col = lane & 15] of each of its tiles
    const double dn1 = (double)(n - 1);
    double* const band = a.band + b * (size_t)V * (W + 1);
#pragma unroll
    for (int q = 0; q < CORR_NACC; ++q) {
        if (q >= nq) continue;
        const int vv = (I + CORR_NACC * panel + q) * 16 + (lane & 15);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int u = I * 16 + (lane >> 4) + 4 * reg;
            const int j = vv - u;
            if (u < V && vv < V && j >= 0 && j <= W) band[(size_t)u * (W + 1) + j] = acc[q][reg] / dn1;
        }
    }
}

// stats[b, 1, v]: the flag of a live variable becomes its pooled sample standard deviation
__global__ __launch_bounds__(256) void k_correlation_sd(size_t total, int V, int W, const double* band, double* stats)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / V, v = i % V;
    double* const p = stats + (b * 2 + 1) * (size_t)V + v;
    if (*p > 0.0) *p = sqrt(band[i * (W + 1)]);
}

__global__ __launch_bounds__(256) void k_correlation_finish(size_t total, int V, int W, int normalise, const double* stats, double* band)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % (W + 1));
    const size_t bc = i / (W + 1), b = bc / V;
    const int c = (int)(bc % V);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double* const sd = stats + (b * 2 + 1) * (size_t)V;
    if (c + j >= V) { band[i] = qnan; return; }
    const double su = sd[c], sv = sd[c + j];
    if (!(su > 0.0) || !(sv > 0.0)) { band[i] = qnan; return; }
    if (normalise) band[i] = j == 0 ? 1.0 : band[i] / (su * sv);
}

// The runs of a band above a threshold (the rule: ensembles.correlation_runs_reference): closed [B, 2, V] = closed_up, closed_down
__global__ __launch_bounds__(256) void k_band_runs(size_t total, int V, int W, const double* band, double threshold, int* up, int* down, uint8_t* closed)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / V;
    const int c = (int)(i % V);
    const double* const row = band + i * (W + 1);
    int nu = 0, nd = 0;
    bool cu = false, cd = false;
    if (row[0] == row[0]) {
        for (int j = 1; j <= W && c + j <= V - 1; ++j) {
            if (!(row[j] >= threshold)) { cd = true; break; }
            ++nd;
        }
        for (int j = 1; j <= W && c - j >= 0; ++j) {
            if (!(row[j - (ptrdiff_t)j * (W + 1)] >= threshold)) { cu = true; break; }
            ++nu;
        }
    }
    up[i] = nu;
    down[i] = nd;
    closed[(b * 2) * (size_t)V + c] = cu ? 1 : 0;
    closed[(b * 2 + 1) * (size_t)V + c] = cd ? 1 : 0;
}

}  // namespace ensemble
