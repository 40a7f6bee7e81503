// Weighted per-column products of a series (the rule: include/geobipy_amd.h gbp_series_weighted and geobipy_amd/ensembles.py
// weighted_reference): per sounding and variable the weighted mean, sd, type-1 quantiles and the weight at or above thresholds of the
// listed rows under INTEGER multiplicities q.  Included by gbp_fdem.hip after gbp_ensemble_ranks.h.
// k_series_weighted<SERIES_PLAIN / SERIES_RASTER>: the two sources of gbp_ensemble_series.h; model u < m = n_used[b] is row rows[b, u]
// (clamped into the rows) with multiplicity q[b, u] (clamped to 0 .. 2^40); a row with q == 0 is never loaded.  The value of a lane is
// series_value (gbp_ensemble_ranks.h): the expression the ranks and the diagnostics evaluate.
// One workgroup of 16 waves per (sounding, tile of T columns); the launch chooses the power of two >= n and T = min(64, WGT_TILE / it):
// keys (f64) and bins (int64) of a tile fill at most 128 KiB of LDS, T = 64 up to 128 listed rows, 8 at 1 024, 2 at 4 096; a 8 KiB
// reduction buffer and T marks follow.  A workgroup pads its own columns to P = the power of two >= m only.
//   total    W = sum q, an integer tree over the workgroup; W == 0 ends here (quantile, stats NaN; above 0).
//   fetch    the participating values of every column into LDS, element i of column c at col[i * T + c] as in k_series_ranks, +inf for
//            q == 0 and behind m.  A non-finite value marks its column and enters as 0.0: the network never compares a NaN.
//   sort     rank_sort on the keys alone: no payload and no stable order are needed, because
//   bins     every participating row fetches its value again, finds its lower bound in the sorted column by binary search and adds q
//            to the int64 bin at that position (ds_add_u64): integer adds commute, ties share the first position of their run.
//   scan     inclusive Kogge-Stone scan of the bins over the positions, in place, the access pattern of the sort (no bank met twice):
//            bins[i] = C(col[i]), the weight at or below the value, monotone.
//   quantile binary search of the first position with (double)C >= max(p W, 1.0): the value there has positive weight.
//   above    W - C just below the lower bound of the threshold.
//   moments  two passes over the sorted column, the weight of position i being C[i] - C[i - 1] (the summed weight of a run of ties, exact
//            in fp64): thread (j, c) adds positions j, j + 1024 / T, ... in order, then a fixed tree over j.
// No global atomics; every output has one writer; the LDS adds are of integers: a call repeats its own bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gbp_ensemble_ranks.h"

namespace ensemble {

constexpr int WGT_THREADS = RANK_THREADS, WGT_MAX_ROWS = 4096, WGT_MAX_P = 16, WGT_MAX_T = 8, WGT_TILE = 8192;
constexpr long long WGT_MAX_Q = 1ll << 40;

struct WeightedArgs : SeriesArgs {       // (no segments: seg_* NULL, M_max = reach = 0)
    int n;                            // listed rows per sounding
    const int* rows;                  // [B, n]
    const int* n_used;                // [B]
    const long long* q;               // [B, n]
    int n_p, n_t;
    long long* total;                 // [B]
    double* quantile;                 // NULL or [B, n_p, V]
    long long* above;                 // NULL or [B, n_t, V]
    double* stats;                    // NULL or [B, 2, V]
    int T, P;                         // columns per workgroup, padded length of n (powers of two, T * P <= WGT_TILE)
    double p[WGT_MAX_P];
    double thr[WGT_MAX_T];
};

constexpr size_t weighted_lds_bytes(int T, int P)
{
    return (size_t)T * P * (sizeof(double) + sizeof(long long)) + (size_t)WGT_THREADS * sizeof(double) + (size_t)T * sizeof(int);
}

template <int SOURCE>
__global__ __launch_bounds__(WGT_THREADS) void k_series_weighted(WeightedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double wgt_lds[];
    const int T = a.T, tshift = __builtin_ctz(T);
    double* const col = wgt_lds;                                       // [P][T]
    long long* const bins = (long long*)(col + (size_t)T * a.P);       // [P][T]
    double* const red = (double*)(bins + (size_t)T * a.P);             // [WGT_THREADS]
    long long* const redq = (long long*)red;
    int* const bad = (int*)(red + WGT_THREADS);                        // [T]
    const int V = a.V, tiles = (V + T - 1) / T, tid = threadIdx.x;
    const size_t b = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x % tiles), v0 = tile * T;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int m = __builtin_amdgcn_readfirstlane(min(max(a.n_used[b], 0), a.n));
    const long long* const qb = a.q + b * (size_t)a.n;
    const int* const rb = a.rows + b * (size_t)a.n;
    auto weight = [&](int i) { const long long qi = qb[i]; return qi < 0 ? 0ll : (qi > WGT_MAX_Q ? WGT_MAX_Q : qi); };
    auto value = [&](int i, int v) { return series_value<SOURCE>(a, series_row(a, b, rb[i]), v, SOURCE == SERIES_RASTER ? a.z[v] : 0.0); };
    auto finite = [](double x) { return (__double2hiint(x) & 0x7ff00000) != 0x7ff00000; };

    // ---- total
    long long w = 0;
    for (int i = tid; i < m; i += WGT_THREADS) w += weight(i);
    redq[tid] = w;
    __syncthreads();
    for (int h = WGT_THREADS >> 1; h > 0; h >>= 1) {
        if (tid < h) redq[tid] += redq[tid + h];
        __syncthreads();
    }
    const long long W = redq[0];
    __syncthreads();                                                   // (red is used again below)
    if (tile == 0 && tid == 0) a.total[b] = W;
    const int nq = a.quantile != nullptr ? a.n_p : 0, nt = a.above != nullptr ? a.n_t : 0;
    if (nq == 0 && nt == 0 && a.stats == nullptr) return;
    if (W == 0) {
        for (int e = tid; e < (nq + nt + 2) << tshift; e += WGT_THREADS) {
            const int c = e & (T - 1), r = e >> tshift, v = v0 + c;
            if (v >= V) continue;
            if (r < nq) a.quantile[(b * nq + r) * (size_t)V + v] = qnan;
            else if (r < nq + nt) a.above[(b * nt + (r - nq)) * (size_t)V + v] = 0;
            else if (a.stats != nullptr) a.stats[(b * 2 + (r - nq - nt)) * (size_t)V + v] = qnan;
        }
        return;
    }
    int P = 1;
    while (P < m) P <<= 1;                                             // this sounding's padded length: m <= P <= a.P
    const int cells = P << tshift, live = m << tshift;

    // ---- fetch
    for (int c = tid; c < T; c += WGT_THREADS) bad[c] = 0;
    __syncthreads();
    for (int e = tid; e < cells; e += WGT_THREADS) {
        const int c = e & (T - 1), i = e >> tshift, vc = min(v0 + c, V - 1);
        double x = (double)INFINITY;
        if (i < m && weight(i) > 0) {
            x = value(i, vc);
            if (!finite(x)) { bad[c] = 1; x = 0.0; }
        }
        col[e] = x;
        bins[e] = 0;
    }
    __syncthreads();
    rank_sort(col, T, P);

    // ---- bins: the weight of every participating row at the lower bound of its value
    for (int e = tid; e < live; e += WGT_THREADS) {
        const int c = e & (T - 1), i = e >> tshift, vc = min(v0 + c, V - 1);
        const long long qi = weight(i);
        if (qi == 0) continue;
        double x = value(i, vc);
        if (!finite(x)) x = 0.0;
        int lo = 0, hi = m - 1;                                        // (the value is in the column: its lower bound is below m)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (col[((size_t)mid << tshift) + c] < x) lo = mid + 1; else hi = mid;
        }
        atomicAdd((unsigned long long*)&bins[((size_t)lo << tshift) + c], (unsigned long long)qi);
    }
    __syncthreads();

    // ---- scan: bins[i] = the weight at or below col[i], i < m
    for (int d = 1; d < m; d <<= 1) {
        long long add[WGT_TILE / WGT_THREADS];
#pragma unroll
        for (int r = 0; r < WGT_TILE / WGT_THREADS; ++r) {
            const int e = tid + r * WGT_THREADS;
            add[r] = e < live && (e >> tshift) >= d ? bins[e - (d << tshift)] : 0;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < WGT_TILE / WGT_THREADS; ++r) {
            const int e = tid + r * WGT_THREADS;
            if (add[r] != 0) bins[e] += add[r];
        }
        __syncthreads();
    }

    // ---- quantiles: the first position whose cumulative weight reaches max(p W, 1)
    for (int e = tid; e < nq << tshift; e += WGT_THREADS) {
        const int c = e & (T - 1), r = e >> tshift, v = v0 + c;
        if (v >= V) continue;
        const double target = fmax(a.p[r] * (double)W, 1.0);
        int lo = 0, hi = m - 1;                                        // (C[m - 1] = W reaches every target)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)bins[((size_t)mid << tshift) + c] >= target) hi = mid; else lo = mid + 1;
        }
        a.quantile[(b * nq + r) * (size_t)V + v] = bad[c] ? qnan : col[((size_t)lo << tshift) + c];
    }

    // ---- above: the weight of the values >= a threshold
    for (int e = tid; e < nt << tshift; e += WGT_THREADS) {
        const int c = e & (T - 1), r = e >> tshift, v = v0 + c;
        if (v >= V) continue;
        const double t = a.thr[r];
        int lo = 0, hi = m;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (col[((size_t)mid << tshift) + c] < t) lo = mid + 1; else hi = mid;
        }
        const long long below = lo > 0 ? bins[((size_t)(lo - 1) << tshift) + c] : 0;
        a.above[(b * nt + r) * (size_t)V + v] = bad[c] ? -1 : W - below;
    }
    if (a.stats == nullptr) return;

    // ---- moments: thread (j, c) owns positions j, j + per, ... of column c; then a tree over j
    const int c = tid & (T - 1), j = tid >> tshift, per = WGT_THREADS >> tshift, v = v0 + c;
    auto column_sum = [&](double mean, bool centred) {
        double s = 0.0;
        for (int i = j; i < m; i += per) {
            const size_t at = ((size_t)i << tshift) + c;
            const long long wi = bins[at] - (i > 0 ? bins[at - T] : 0);
            if (wi == 0) continue;                                     // (q == 0 and padding hold +inf)
            const double x = col[at], d = x - mean;
            s += (double)wi * (centred ? d * d : x);
        }
        __syncthreads();                                               // (the readers of the pass before are done)
        red[tid] = s;
        __syncthreads();
        for (int h = WGT_THREADS >> 1; h >= T; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        return red[c];
    };
    const double mean = column_sum(0.0, false) / (double)W;
    const double var = column_sum(mean, true) / (double)W;
    if (j == 0 && v < V) {
        a.stats[(b * 2 + 0) * (size_t)V + v] = bad[c] ? qnan : mean;
        a.stats[(b * 2 + 1) * (size_t)V + v] = bad[c] ? qnan : sqrt(var);
    }
}

}  // namespace ensemble
