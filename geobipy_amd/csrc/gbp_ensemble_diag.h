// Chain diagnostics of regularly spaced series (the rule: include/geobipy_amd.h gbp_series_diagnostics and
// geobipy_amd/ensembles.py diagnostics_reference): per sounding and variable the split-chain autocovariances up to lag L, Geyer's
// initial monotone sequence, tau, ESS, split R-hat and the Monte-Carlo standard error.  Included by gbp_fdem.hip after gbp_ensemble.h.
// k_series_diagnostics<SERIES_PLAIN / SERIES_RASTER>: the two sources of gbp_ensemble_series.h (RASTER: the log10 conductivity at the
// cell centres, built on the fly).
// One workgroup of 16 waves per (sounding, tile of 64 variables); a lane owns a variable, the waves share lags and times.
//   pass 1   every used row once: per segment the sum (-> mean_m), over all segments min, max and a non-finite flag.  A tile whose 64
//            variables are all constant or non-finite ends here (the deep cells of a depth axis).
//   pass 2   per segment the centred rows go through a ring of R = CH + LPAD rows x 64 doubles in LDS (LPAD = 16 * lag groups >= L + 1,
//            CH = the chunk of times worked on between two refills); rows past the segment's end are zero, so every time takes every
//            lag.  The ring's first MIRROR rows are stored a second time behind its end: a run of up to MIRROR + 1 rows that starts
//            anywhere in the ring is contiguous, so the reads of a block are one base address and immediate offsets.  A row is
//            rastered twice in all (pass 1 and pass 2), whatever L is.
//            Wave w = tg * nlg + lg owns the 16 lags of lag group lg and every ntg-th block of 8 times: 8 centred values and 16
//            running sums sit in registers, 23 lagged values stream past them -- 31 ds_read_b64 for 128 FMAs.  The sums run over the
//            segments too: only their total enters the rule.
//   finish   the sums of the time groups are added in a fixed order through LDS; wave 0 walks the lags of its 64 variables.
// No atomics; every sum has one order, so a run repeats its own bits.  LDS: DIAG_LDS_BYTES whatever L is (one workgroup per CU, four
// waves per SIMD; the ring for L = 255 needs it, and the finish needs 128 KiB for the 16 waves' sums).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gbp_ensemble_series.h"

namespace ensemble {

constexpr int DIAG_WAVES = 16, DIAG_TB = 8, DIAG_LG = 16, DIAG_MIRROR = DIAG_TB + DIAG_LG - 2;       // 22: a run is at most 23 rows
constexpr int DIAG_RING_ROWS = 296;                                   // R + MIRROR <= 296: L = 255 leaves CH = 16
constexpr size_t DIAG_LDS_BYTES = (size_t)(SERIES_MAX_M + DIAG_RING_ROWS) * 64 * sizeof(double);     // 159 744 B <= 160 KiB

struct DiagArgs : SeriesArgs {           // reach: max_lag
    double* stats;                    // [B, 6, V]
    int* pairs;                       // [B, V]
    double* rho;                      // NULL or [B, max_lag + 1, V]
};

// The value of variable v (this lane's; RASTER: the centre zc) in row `row` of sounding b; one wave per row.  The row is clamped and
// the one centre counted here, in the order this kernel always had: through series_row and layers<1> the same rule compiles to
// other code.
template <int SOURCE>
__device__ __forceinline__ double diag_fetch(const DiagArgs& a, size_t b, int row, int v, int lane, double zc)
{
    row = min(max(row, 0), a.n_rows - 1);                              // (series_row's clamp)
    const size_t src = b * a.n_rows + row;
    if (SOURCE == SERIES_PLAIN) return a.x[src * (size_t)a.V + v];
    const Slot q = slot_load(a, src, lane);
    int layer = 0;                                                     // (layers<1>)
    for (int l = 0; l < q.k - 1; ++l) {
        const double el = __hiloint2double(__builtin_amdgcn_readlane(q.e_hi, l), __builtin_amdgcn_readlane(q.e_lo, l));
        layer += el <= zc ? 1 : 0;
    }
    return __shfl(q.s, layer, 64);
}

template <int SOURCE>
__global__ __launch_bounds__(DIAG_WAVES * 64) void k_series_diagnostics(DiagArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double diag_lds[];
    double* const sh_mean = diag_lds;                                  // [SERIES_MAX_M][64]
    double* const ring = diag_lds + SERIES_MAX_M * 64;                 // [DIAG_RING_ROWS][64]; pass 1 and the finish use it as scratch
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
    double* const st = a.stats + b * 6 * (size_t)V;
    if (M <= 0 || N < 4) {
        if (w == 0 && own) {
            for (int q = 0; q < 6; ++q) st[(size_t)q * V + v] = qnan;
            a.pairs[b * V + v] = 0;
        }
        if (a.rho != nullptr && own)
            for (int l = w; l <= a.reach; l += DIAG_WAVES) a.rho[(b * (a.reach + 1) + l) * (size_t)V + v] = qnan;
        return;
    }
    int L = min(a.reach, N - 1);
    L -= (L & 1) ? 0 : 1;
    const int nlg = (L + DIAG_LG) / DIAG_LG, LPAD = nlg * DIAG_LG, ntg = DIAG_WAVES / nlg;
    const int CH = min((DIAG_RING_ROWS - DIAG_MIRROR - LPAD) & ~(DIAG_TB - 1), DIAG_TB * ntg * 4);
    const int R = CH + LPAD;
    const int lg = w % nlg, tg = w / nlg;
    const int* const seg0 = series_starts(a, b);
    const double zc = SOURCE == SERIES_RASTER ? a.z[vc] : 0.0;

    // ---- pass 1: sums, min, max, non-finite
    double mn = (double)INFINITY, mx = -(double)INFINITY, gsum = 0.0;
    int bad = 0;
    for (int m = 0; m < M; ++m) {
        const int r0 = __builtin_amdgcn_readfirstlane(seg0[m]);
        double s = 0.0, lo = (double)INFINITY, hi = -(double)INFINITY;
        int nf = 0;
        for (int t = w; t < N; t += DIAG_WAVES) {
            const double x = diag_fetch<SOURCE>(a, b, r0 + t, vc, lane, zc);
            s += x;
            lo = fmin(lo, x);
            hi = fmax(hi, x);
            nf |= (__double2hiint(x) & 0x7ff00000) == 0x7ff00000 ? 1 : 0;
        }
        ring[(0 * DIAG_WAVES + w) * 64 + lane] = s;
        ring[(1 * DIAG_WAVES + w) * 64 + lane] = lo;
        ring[(2 * DIAG_WAVES + w) * 64 + lane] = hi;
        ring[(3 * DIAG_WAVES + w) * 64 + lane] = (double)nf;
        __syncthreads();
        if (w == 0) {
            double t = 0.0;
            for (int u = 0; u < DIAG_WAVES; ++u) {
                t += ring[(0 * DIAG_WAVES + u) * 64 + lane];
                mn = fmin(mn, ring[(1 * DIAG_WAVES + u) * 64 + lane]);
                mx = fmax(mx, ring[(2 * DIAG_WAVES + u) * 64 + lane]);
                bad |= ring[(3 * DIAG_WAVES + u) * 64 + lane] != 0.0 ? 1 : 0;
            }
            const double mean = t / (double)N;
            sh_mean[m * 64 + lane] = mean;
            gsum += mean;
        }
        __syncthreads();
    }
    const bool constant = !bad && mn == mx;                            // (wave 0's lanes hold the truth; the others are not asked)
    if (w == 0) {
        const unsigned long long live = __ballot(own && !bad && !constant);
        if (lane == 0) ring[0] = live != 0ull ? 1.0 : 0.0;
    }
    __syncthreads();
    const bool any_live = ring[0] != 0.0;
    __syncthreads();

    // ---- pass 2: lag products
    double acc[DIAG_LG];
#pragma unroll
    for (int j = 0; j < DIAG_LG; ++j) acc[j] = 0.0;
    if (any_live) {
        const bool worker = tg < ntg;
        for (int m = 0; m < M; ++m) {
            const int r0 = __builtin_amdgcn_readfirstlane(seg0[m]);
            const double mean = sh_mean[m * 64 + lane];
            auto stage = [&](int t_begin, int t_end) {                 // rows t_begin .. t_end - 1 of the segment into the ring
                for (int t = t_begin + w; t < t_end; t += DIAG_WAVES) {
                    const double d = t < N ? diag_fetch<SOURCE>(a, b, r0 + t, vc, lane, zc) - mean : 0.0;
                    const int p = t % R;
                    ring[p * 64 + lane] = d;
                    if (p < DIAG_MIRROR) ring[(R + p) * 64 + lane] = d;
                }
            };
            stage(0, R);
            __syncthreads();
            for (int c0 = 0; c0 < N; c0 += CH) {
                if (worker) {
                    for (int t0 = c0 + DIAG_TB * tg; t0 < min(c0 + CH, N); t0 += DIAG_TB * ntg) {
                        const double* const pa = ring + (t0 % R) * 64 + lane;
                        const double* const py = ring + ((t0 + lg * DIAG_LG) % R) * 64 + lane;
                        double x[DIAG_TB];
#pragma unroll
                        for (int i = 0; i < DIAG_TB; ++i) x[i] = pa[i * 64];
#pragma unroll
                        for (int r = 0; r < DIAG_TB + DIAG_LG - 1; ++r) {
                            const double y = py[r * 64];
#pragma unroll
                            for (int i = 0; i < DIAG_TB; ++i) {
                                const int j = r - i;
                                if (j >= 0 && j < DIAG_LG) acc[j] = __builtin_fma(x[i], y, acc[j]);
                            }
                        }
                    }
                }
                __syncthreads();
                if (c0 + CH < N) {
                    stage(c0 + R, c0 + R + CH);
                    __syncthreads();
                }
            }
        }
    }

    // ---- finish: the time groups' sums in a fixed order, then the walk over the lags
    if (any_live) {
#pragma unroll
        for (int j = 0; j < DIAG_LG; ++j) ring[(w * DIAG_LG + j) * 64 + lane] = acc[j];
    }
    __syncthreads();
    if (w != 0) {
        if (a.rho != nullptr && own)                                   // (beyond L: NaN; wave 0 writes 0 .. L)
            for (int l = L + w; l <= a.reach; l += DIAG_WAVES - 1) a.rho[(b * (a.reach + 1) + l) * (size_t)V + v] = qnan;
        return;
    }
    const double dM = (double)M, dN = (double)N, bessel = dN / (dN - 1.0);
    const double gm = gsum / dM;
    double out[6];
    int np = 0;
    double* const rho = a.rho != nullptr && own ? a.rho + b * (a.reach + 1) * (size_t)V + v : nullptr;
    if (bad || constant) {
        out[0] = bad ? qnan : mn;
        out[1] = bad ? qnan : 0.0;
        out[2] = out[3] = out[4] = out[5] = qnan;
        if (rho != nullptr)
            for (int l = 0; l <= L; ++l) rho[(size_t)l * V] = qnan;
    } else {
        auto acov = [&](int l) {                                       // (1/M) sum_m acov_m(l) * N / (N - 1)
            double t = 0.0;
            for (int g = 0; g < ntg; ++g) t += ring[((g * nlg + l / DIAG_LG) * DIAG_LG + (l % DIAG_LG)) * 64 + lane];
            return t / dN / dM * bessel;
        };
        double bn = 0.0;
        if (M > 1) {
            for (int m = 0; m < M; ++m) {
                const double d = sh_mean[m * 64 + lane] - gm;
                bn += d * d;
            }
            bn /= dM - 1.0;
        }
        const double W = acov(0);
        const double vp = W * (dN - 1.0) / dN + bn;
        double S = 0.0, prev = 0.0;
        bool open = true;
        if (rho != nullptr) rho[0] = 1.0;
        for (int kk = 0; 2 * kk + 1 <= L; ++kk) {
            const double r_even = kk == 0 ? 1.0 : 1.0 - (W - acov(2 * kk)) / vp;
            const double r_odd = 1.0 - (W - acov(2 * kk + 1)) / vp;
            if (rho != nullptr) {
                if (kk > 0) rho[(size_t)(2 * kk) * V] = r_even;
                rho[(size_t)(2 * kk + 1) * V] = r_odd;
            }
            const double P = r_even + r_odd;
            if (open) {
                if (kk == 0) { S = prev = P; np = 1; }
                else if (P > 0.0) { prev = fmin(prev, P); S += prev; np += 1; }
                else open = false;
            }
            if (!open && rho == nullptr) break;
        }
        const double total = dM * dN;
        const double tau = fmax(2.0 * S - 1.0, 1.0 / log10(total));
        const double ess = total / tau;
        out[0] = gm;
        out[1] = sqrt(vp);
        out[2] = sqrt(vp / W);
        out[3] = tau;
        out[4] = ess;
        out[5] = sqrt(vp / ess);
    }
    if (own) {
        for (int q = 0; q < 6; ++q) st[(size_t)q * V + v] = out[q];
        a.pairs[b * V + v] = np;
    }
}

}  // namespace ensemble
