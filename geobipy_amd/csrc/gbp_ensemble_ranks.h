// Ranks of regularly spaced series (the rule: include/geobipy_amd.h gbp_series_ranks and geobipy_amd/ensembles.py
// rank_counts_reference): per sounding and variable, for every used row the number of used values below it (less) and not above it
// (leq), ties included, and order statistics of the column.  Included by gbp_fdem.hip after gbp_ensemble_diag.h.
// k_series_ranks<SERIES_PLAIN / SERIES_RASTER, FOLD>: the two sources of gbp_ensemble_series.h.  RASTER: a lane owns one (row, centre)
// and counts that row's interfaces itself -- layer = #{l < k - 1 : edges[l] <= z}, the count gbp_ensemble_series.h states -- then takes
// log10 of the layer's stored value: slot_load's value, the same function of the same double.  (slot_load spends a wave on a row; with
// a tile of 4 columns at 4 096 rows 60 of its 64 lanes would hold nothing this kernel reads.)
// One workgroup of 16 waves per (sounding, tile of T columns); the launch chooses P = the power of two >= n_rows and T = min(64,
// RANK_TILE_DOUBLES / P), so the tile's columns fill at most 128 KiB of LDS: T = 64 up to 256 rows, 4 at 4 096, 1 at 16 384.
//   unused   a row in no segment: less = leq = -1, x_out = NaN.
//   fetch    the n = M N used values of every column into LDS, element i of column c at col[i * T + c] (a wave reads and writes
//            consecutive doubles: ds_read_b64 meets no bank twice), +inf behind them up to P.  A non-finite value marks its column and
//            enters as 0.0, so the network below never compares a NaN.
//   sort     bitonic network on the keys alone, all T columns at once: a thread owns the compare-exchange of elements i and i | j.
//            The padding is +inf and ends behind every value, folded +inf included: the first n sorted elements are the column.
//   order    the two order statistics per probability, copied from the sorted column.
//   FOLD     med = 0.5 (s[(n - 1) / 2] + s[n / 2]) per column, then fetch again as |x - med| and sort again.
//   counts   every used row's value is fetched a third time by the same expression; less and leq are the lower and upper bound of
//            two binary searches in col[0 .. n).  No index array; ties by construction.
// No atomics (the column marks are plain LDS stores of one value); every output has one writer: a call repeats its own bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gbp_ensemble_series.h"

namespace ensemble {

constexpr int RANK_THREADS = 1024, RANK_MAX_ROWS = 16384, RANK_MAX_P = 16, RANK_TILE_DOUBLES = 16384;

struct RankArgs : SeriesArgs {           // reach: n_p
    int* less;                        // NULL (with leq) or [B, n_rows, V]
    int* leq;
    double* order;                    // NULL or [B, n_p, 2, V]
    double* x_out;                    // NULL or [B, n_rows, V]
    int T, P;                         // columns per workgroup, padded column length (powers of two, T * P <= RANK_TILE_DOUBLES)
    double p[RANK_MAX_P];
};

constexpr size_t rank_lds_bytes(int T, int P) { return ((size_t)T * P + T) * sizeof(double) + (size_t)T * sizeof(int); }

// The value of variable v in source row `src` (series_row) of the series, one per lane: what k_series_weighted shares.
template <int SOURCE>
__device__ __forceinline__ double series_value(const SeriesArgs& a, size_t src, int v, double zc)
{
    if (SOURCE == SERIES_PLAIN) return a.x[src * (size_t)a.V + v];
    const int k = min(max(a.ens_k[src], 0), a.K);
    if (k == 0) return __longlong_as_double(0x7ff8000000000000ll);
    const double* const e = a.ens_edges + src * a.K;
    int layer = 0;
    for (int l = 0; l < k - 1; ++l) layer += e[l] <= zc ? 1 : 0;
    return log10(a.ens_sigma[src * a.K + layer]);
}

// The value of variable v in row `row` of sounding b, one per lane.
template <int SOURCE>
__device__ __forceinline__ double rank_fetch(const RankArgs& a, size_t b, int row, int v, double zc)
{
    return series_value<SOURCE>(a, series_row(a, b, row), v, zc);
}

// col[i * T + c], i < P, ascending per column c
__device__ __forceinline__ void rank_sort(double* col, int T, int P)
{
    const int tshift = __builtin_ctz(T), half = (P >> 1) << tshift;
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int e = threadIdx.x; e < half; e += RANK_THREADS) {
                const int c = e & (T - 1), q = e >> tshift;
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                double* const pa = col + ((size_t)i << tshift) + c;
                double* const pb = col + ((size_t)(i | j) << tshift) + c;
                const double x = *pa, y = *pb;
                const bool up = (i & kk) == 0;
                if (up ? x > y : x < y) { *pa = y; *pb = x; }
            }
            __syncthreads();
        }
    }
}

template <int SOURCE, bool FOLD>
__global__ __launch_bounds__(RANK_THREADS) void k_series_ranks(RankArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double rank_lds[];
    const int T = a.T, P = a.P, tshift = __builtin_ctz(T);
    double* const col = rank_lds;                                      // [P][T]
    double* const med = rank_lds + (size_t)T * P;                      // [T]
    int* const bad = (int*)(med + T);                                  // [T]
    const int V = a.V, tiles = (V + T - 1) / T, nq = a.reach;
    const size_t b = blockIdx.x / tiles;
    const int v0 = (int)(blockIdx.x % tiles) * T;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const Segments seg = series_segments(a, b);
    const int* const seg0 = series_starts(a, b);
    const bool counts = a.less != nullptr && a.leq != nullptr;
    // (n <= n_rows <= P keeps the column inside its LDS: overlapping segments are the caller's error and count as no segments)
    const bool empty = seg.M <= 0 || seg.N < 4 || (long long)seg.M * seg.N > (long long)a.n_rows;
    const int M = empty ? 0 : seg.M, N = seg.N, n = M * N;
    const size_t rows0 = b * (size_t)a.n_rows;

    // ---- the rows in no segment
    if (counts || a.x_out != nullptr) {
        for (int e = threadIdx.x; e < a.n_rows << tshift; e += RANK_THREADS) {
            const int c = e & (T - 1), t = e >> tshift, v = v0 + c;
            bool used = false;
            for (int m = 0; m < M; ++m) used |= t >= seg0[m] && t < seg0[m] + N;
            if (used || v >= V) continue;
            const size_t at = (rows0 + t) * (size_t)V + v;
            if (counts) { a.less[at] = -1; a.leq[at] = -1; }
            if (a.x_out != nullptr) a.x_out[at] = qnan;
        }
    }
    if (empty) {
        if (a.order != nullptr)
            for (int e = threadIdx.x; e < (2 * nq) << tshift; e += RANK_THREADS) {
                const int c = e & (T - 1), v = v0 + c;
                if (v < V) a.order[(b * (2 * nq) + (e >> tshift)) * (size_t)V + v] = qnan;
            }
        return;
    }

    auto row_of = [&](int i) { return seg0[i / N] + i % N; };           // used row i = m N + t
    auto stage = [&](bool fold) {                                      // the columns into LDS, padded; the first time: marks and x_out
        for (int e = threadIdx.x; e < P << tshift; e += RANK_THREADS) {
            const int c = e & (T - 1), i = e >> tshift, v = v0 + c, vc = min(v, V - 1);
            double x = (double)INFINITY;
            if (i < n) {
                const int row = row_of(i);
                x = rank_fetch<SOURCE>(a, b, row, vc, SOURCE == SERIES_RASTER ? a.z[vc] : 0.0);
                const bool finite = (__double2hiint(x) & 0x7ff00000) != 0x7ff00000;
                if (!fold) {
                    if (a.x_out != nullptr && v < V) a.x_out[series_row(a, b, row) * (size_t)V + v] = x;
                    if (!finite) bad[c] = 1;
                }
                x = !finite ? 0.0 : (fold ? fabs(x - med[c]) : x);
            }
            col[e] = x;
        }
    };

    for (int c = threadIdx.x; c < T; c += RANK_THREADS) bad[c] = 0;
    __syncthreads();
    stage(false);
    __syncthreads();
    if (a.order == nullptr && !counts) return;
    rank_sort(col, T, P);

    // ---- order statistics (before any folding)
    if (a.order != nullptr) {
        for (int e = threadIdx.x; e < (2 * nq) << tshift; e += RANK_THREADS) {
            const int c = e & (T - 1), qh = e >> tshift, v = v0 + c;
            if (v >= V) continue;
            const int lo = (int)floor((double)(n - 1) * a.p[qh >> 1]);
            const int at = min(max(lo + (qh & 1), 0), n - 1);
            a.order[(b * (2 * nq) + qh) * (size_t)V + v] = bad[c] ? qnan : col[((size_t)at << tshift) + c];
        }
    }
    if (!counts) return;

    if (FOLD) {
        for (int c = threadIdx.x; c < T; c += RANK_THREADS)
            med[c] = 0.5 * (col[((size_t)((n - 1) / 2) << tshift) + c] + col[((size_t)(n / 2) << tshift) + c]);
        __syncthreads();
        stage(true);
        __syncthreads();
        rank_sort(col, T, P);
    }

    // ---- counts: lower and upper bound of every used value in its sorted column
    for (int e = threadIdx.x; e < n << tshift; e += RANK_THREADS) {
        const int c = e & (T - 1), i = e >> tshift, v = v0 + c;
        if (v >= V) continue;
        const int row = row_of(i);
        const size_t at = series_row(a, b, row) * (size_t)V + v;
        if (bad[c]) { a.less[at] = -1; a.leq[at] = -1; continue; }
        double x = rank_fetch<SOURCE>(a, b, row, v, SOURCE == SERIES_RASTER ? a.z[v] : 0.0);
        if (FOLD) x = fabs(x - med[c]);
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (col[((size_t)mid << tshift) + c] < x) lo = mid + 1; else hi = mid;
        }
        const int less = lo;
        hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (col[((size_t)mid << tshift) + c] <= x) lo = mid + 1; else hi = mid;
        }
        a.less[at] = less;
        a.leq[at] = lo;
    }
}

}  // namespace ensemble
