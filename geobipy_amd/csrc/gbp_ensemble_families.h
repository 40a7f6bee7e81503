// Families of kept models (the rules: include/geobipy_amd.h gbp_ensemble_distance / gbp_distance_families and
// geobipy_amd/families.py distance_reference / families_reference).  Included by gbp_fdem.hip after gbp_ensemble_corr.h.
//   k_layered_distance<LOG>   the RMS difference in decades of two layered models over a depth window, the exact integral of the squared
//                             difference of two piecewise-constant functions.  One workgroup of 256 threads per (sounding, 16 x 16 tile
//                             of pairs, tile column >= tile row).  The tile's 32 models are staged once in LDS -- per model K edges (the
//                             k - 1 interfaces, then +inf) and K values (the k values, log10 taken once per staged layer, then NaN), a
//                             row of 2 K + 1 doubles: the odd stride puts the 16 column models a half wave reads at one pointer on 16
//                             different bank pairs -- and each thread merges one pair with two pointers: O(k_i + k_j), no depth axis.
//                             The thread writes its value to (u, v) and (v, u): symmetric bit for bit.  The diagonal of a present
//                             model is written as 0.0; an absent model (row outside the slots, k <= 0) gives NaN.  LOG: mu = ln(q / p), as log1p((q - p) / p).
//   k_layered_cross_distance<LOG>  the same distance (layered_pair: one merge for both kernels, the same bits) between the models of a
//                             sounding and those of its partner sounding (gbp_ensemble_cross_distance).  The same
//                             staging -- rows 0 .. 15 the sounding's models, 16 .. 31 the partner's -- over all nt x nt tiles: nothing is
//                             symmetric, there is no diagonal, and identical models are 0.0 apart by arithmetic.  A partner outside
//                             0 .. S - 1 gives a slab of NaN.  The kernel writes every entry.
//   k_distance_families       k-medoids on a distance matrix, every stage q = 1 .. q_max of a sounding in one launch by one workgroup of
//                             256 threads.  Thread t owns columns t, t + 256, ...: it walks j upward over row j's entry of its own
//                             column (a wave reads 64 consecutive doubles) and its sum keeps the rule's order.  Labels and nearest
//                             distances live in LDS (12 n bytes); a thread keeps the running best of every family for its own columns in
//                             registers (an unrolled select, never an indexed private array), a wave reduces (value, index) with
//                             shuffles and the four waves meet in LDS.  Every output is an integer or a copy of an input double.
// No atomics; every sum has one order, so a call repeats its own bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gbp_ensemble_series.h"

namespace ensemble {

constexpr int FAM_TILE = 16, FAM_THREADS = 256, FAM_MAX_Q = 8, FAM_WAVES = FAM_THREADS / 64;

__host__ __device__ constexpr int family_stride(int K) { return 2 * K + 1; }             // doubles per staged model
inline size_t distance_lds_bytes(int K) { return (size_t)2 * FAM_TILE * family_stride(K) * sizeof(double); }      // 33 024 B at K = 64
inline size_t families_lds_bytes(int n) { return (size_t)n * (sizeof(double) + sizeof(int)); }                    // 49 152 B at n = 4096

struct DistanceArgs {
    int n_slots, K, n;
    const int* ens_k;
    const double* ens_edges;
    const double* ens_sigma;
    const int* rows;                  // [B, n]
    double z0, z1, inv_mu;            // 1 / mu([z0, z1])
    int log10, squared, ntp;          // tile pairs per sounding: nt (nt + 1) / 2
    double* dist;                     // [B, n, n]
};

// The distance of two staged models (rows of 2 K + 1 doubles: K edges, K values) with ki, kj >= 1 layers: the merge of the header's
// rule, one order of the sum.  Both kernels call it, so a pair of models gives the same bits through either entry.
template <bool LOG>
__device__ __forceinline__ double layered_pair(const double* ei, const double* ej, int ki, int kj, int K, double z0, double z1, double inv_mu,
                                               int squared)
{
    const double *ai = ei + K, *aj = ej + K;
    int li = 0, lj = 0;
    for (int l = 0; l < ki - 1; ++l) li += ei[l] <= z0 ? 1 : 0;
    for (int l = 0; l < kj - 1; ++l) lj += ej[l] <= z0 ? 1 : 0;
    double p = z0, acc = 0.0;
    for (int step = 0; step < 2 * K + 2 && p < z1; ++step) {           // (at most k_i + k_j - 1 segments: the cap only guards malformed edges)
        const double ni = li < ki - 1 ? ei[li] : (double)INFINITY, nj = lj < kj - 1 ? ej[lj] : (double)INFINITY;
        const double q = fmin(fmin(ni, nj), z1);
        const double d = ai[li] - aj[lj];
        const double mu = LOG ? log1p((q - p) / p) : q - p;              // (ln(q / p), to a few U relative however thin the segment)
        acc += mu * (d * d);
        li += ni == q ? 1 : 0;
        lj += nj == q ? 1 : 0;
        p = q;
    }
    const double d2 = acc * inv_mu;
    return squared ? d2 : sqrt(d2);
}

template <bool LOG>
__global__ __launch_bounds__(FAM_THREADS) void k_layered_distance(DistanceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double fam_lds[];
    __shared__ int sk[2 * FAM_TILE];
    const int t = threadIdx.x, K = a.K, n = a.n, S = family_stride(K);
    const int nt = (n + FAM_TILE - 1) / FAM_TILE;
    const size_t b = blockIdx.x / (unsigned)a.ntp;
    int rem = (int)(blockIdx.x % (unsigned)a.ntp), tr = 0;
    while (rem >= nt - tr) { rem -= nt - tr; ++tr; }                   // (tile row tr holds the nt - tr tiles tc = tr .. nt - 1)
    const int tc = tr + rem;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    // ---- stage: model m < 16 is tr * 16 + m, model m >= 16 is tc * 16 + m - 16
    for (int idx = t; idx < 2 * FAM_TILE * K; idx += FAM_THREADS) {
        const int m = idx / K, l = idx - m * K;
        const int u = (m < FAM_TILE ? tr : tc) * FAM_TILE + (m & (FAM_TILE - 1));
        const int r = a.rows[b * n + min(u, n - 1)];
        const bool present = u < n && r >= 0 && r < a.n_slots;
        const size_t src = b * a.n_slots + (size_t)min(max(r, 0), a.n_slots - 1);      // (clamped before any load)
        const int k = present ? min(max(a.ens_k[src], 0), K) : 0;
        if (l == 0) sk[m] = k;
        double* const row = fam_lds + m * S;
        row[l] = l < k - 1 ? a.ens_edges[src * K + l] : (double)INFINITY;
        const double s = l < k ? a.ens_sigma[src * K + l] : qnan;
        row[K + l] = l < k && a.log10 ? log10(s) : s;
    }
    __syncthreads();

    const int i = t >> 4, j = t & (FAM_TILE - 1);
    const int u = tr * FAM_TILE + i, v = tc * FAM_TILE + j;
    if (u >= n || v >= n || (tr == tc && u > v)) return;               // (a diagonal tile: its upper triangle, mirrored below)
    const int ki = sk[i], kj = sk[FAM_TILE + j];
    double* const out = a.dist + b * (size_t)n * n;
    double value;
    if (ki == 0 || kj == 0) value = qnan;
    else if (u == v) value = 0.0;
    else value = layered_pair<LOG>(fam_lds + i * S, fam_lds + (FAM_TILE + j) * S, ki, kj, K, a.z0, a.z1, a.inv_mu, a.squared);
    out[(size_t)u * n + v] = value;
    if (u != v) out[(size_t)v * n + u] = value;
}

struct CrossDistanceArgs {
    int S, n_slots, K, n;
    const int* ens_k;
    const double* ens_edges;
    const double* ens_sigma;
    const int* rows;                  // [S, n]
    const int* partner;               // [S]
    double z0, z1, inv_mu;
    int log10, squared, nt2;          // tiles per sounding: nt * nt
    double* dist;                     // [S, n, n]
};

template <bool LOG>
__global__ __launch_bounds__(FAM_THREADS) void k_layered_cross_distance(CrossDistanceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double fam_lds[];
    __shared__ int sk[2 * FAM_TILE];
    const int t = threadIdx.x, K = a.K, n = a.n, S = family_stride(K);
    const int nt = (n + FAM_TILE - 1) / FAM_TILE;
    const size_t b = blockIdx.x / (unsigned)a.nt2;
    const int rem = (int)(blockIdx.x % (unsigned)a.nt2), tr = rem / nt, tc = rem - tr * nt;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int i = t >> 4, j = t & (FAM_TILE - 1);
    const int u = tr * FAM_TILE + i, v = tc * FAM_TILE + j;
    double* const out = a.dist + b * (size_t)n * n;
    const int pb = a.partner[b];
    if (pb < 0 || pb >= a.S) {                                         // (the same for the whole workgroup: nobody waits at the barrier)
        if (u < n && v < n) out[(size_t)u * n + v] = qnan;
        return;
    }

    // ---- stage: model m < 16 is tr * 16 + m of sounding b, model m >= 16 is tc * 16 + m - 16 of its partner
    for (int idx = t; idx < 2 * FAM_TILE * K; idx += FAM_THREADS) {
        const int m = idx / K, l = idx - m * K;
        const int w = (m < FAM_TILE ? tr : tc) * FAM_TILE + (m & (FAM_TILE - 1));
        const size_t sb = m < FAM_TILE ? b : (size_t)pb;
        const int r = a.rows[sb * n + min(w, n - 1)];
        const bool present = w < n && r >= 0 && r < a.n_slots;
        const size_t src = sb * a.n_slots + (size_t)min(max(r, 0), a.n_slots - 1);     // (clamped before any load)
        const int k = present ? min(max(a.ens_k[src], 0), K) : 0;
        if (l == 0) sk[m] = k;
        double* const row = fam_lds + m * S;
        row[l] = l < k - 1 ? a.ens_edges[src * K + l] : (double)INFINITY;
        const double s = l < k ? a.ens_sigma[src * K + l] : qnan;
        row[K + l] = l < k && a.log10 ? log10(s) : s;
    }
    __syncthreads();

    if (u >= n || v >= n) return;
    const int ki = sk[i], kj = sk[FAM_TILE + j];
    double value = qnan;
    if (ki != 0 && kj != 0) value = layered_pair<LOG>(fam_lds + i * S, fam_lds + (FAM_TILE + j) * S, ki, kj, K, a.z0, a.z1, a.inv_mu, a.squared);
    out[(size_t)u * n + v] = value;
}

struct FamilyArgs {
    int n, q_max, max_iter;
    const double* dist;               // [B, n, n]
    const int* n_used;                // [B]
    int* medoid;                      // [B, q_max, q_max]
    int* label;                       // [B, q_max, n]
    double* nearest;                  // [B, q_max, n]
    double* second;                   // [B, q_max, n]
    int* iterations;                  // [B, q_max]
    uint8_t* converged;               // [B, q_max]
    int* n_found;                     // [B]
};

// (value, index) with the smaller value, ties to the lower index, over the wave; every lane gets the result
__device__ __forceinline__ void wave_argmin(double& v, int& i)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

__global__ __launch_bounds__(FAM_THREADS) void k_distance_families(FamilyArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double fam_lds[];
    __shared__ double red_v[FAM_WAVES][FAM_MAX_Q];
    __shared__ int red_i[FAM_WAVES][FAM_MAX_Q];
    __shared__ int smed[FAM_MAX_Q];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = a.n, Q = a.q_max;
    const size_t b = blockIdx.x;
    double* const near = fam_lds;                                      // [n]
    int* const lab = (int*)(fam_lds + n);                              // [n]
    const double* const D = a.dist + b * (size_t)n * n;
    int* const medoid = a.medoid + b * Q * Q;
    int* const label = a.label + b * (size_t)Q * n;
    double* const nearest = a.nearest + b * (size_t)Q * n;
    double* const second = a.second + b * (size_t)Q * n;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll), inf = (double)INFINITY;
    const int m = min(max(a.n_used[b], 0), n);

    // ---- everything "not found"; a thread overwrites only what it wrote here (model j belongs to thread j mod 256, the rest to thread 0)
    for (int st = 0; st < Q; ++st)
        for (int j = t; j < n; j += FAM_THREADS) {
            label[(size_t)st * n + j] = -1;
            nearest[(size_t)st * n + j] = qnan;
            second[(size_t)st * n + j] = qnan;
        }
    if (t == 0) {
        for (int e = 0; e < Q * Q; ++e) medoid[e] = -1;
        for (int st = 0; st < Q; ++st) { a.iterations[b * Q + st] = 0; a.converged[b * Q + st] = 0; }
        a.n_found[b] = 0;
    }
    if (m == 0) return;

    // ---- the prefix must be finite and >= 0
    int bad = 0;
    for (int c = t; c < m; c += FAM_THREADS)
        for (int j = 0; j < m; ++j) {
            const double d = D[(size_t)j * n + c];
            bad |= !(d >= 0.0 && d < inf) ? 1 : 0;
        }
    if (__syncthreads_or(bad)) return;

    // block (value, index) reduction of FAM_MAX_Q candidates at once: wave shuffles, then the four waves in ascending order
    auto reduce = [&](double (&bv)[FAM_MAX_Q], int (&bi)[FAM_MAX_Q], int count) {
#pragma unroll
        for (int p = 0; p < FAM_MAX_Q; ++p) {
            if (p >= count) continue;
            wave_argmin(bv[p], bi[p]);
            if (lane == 0) { red_v[w][p] = bv[p]; red_i[w][p] = bi[p]; }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < FAM_MAX_Q; ++p) {
            if (p >= count) continue;
            bv[p] = red_v[0][p];
            bi[p] = red_i[0][p];
            for (int x = 1; x < FAM_WAVES; ++x) {
                const double ov = red_v[x][p];
                const int oi = red_i[x][p];
                if (ov < bv[p] || (ov == bv[p] && oi < bi[p])) { bv[p] = ov; bi[p] = oi; }
            }
        }
        __syncthreads();                                               // (red_* may be written again)
    };

    int found = 0;
    for (int q = 1; q <= Q; ++q) {
        const int st = q - 1;
        double bv[FAM_MAX_Q];
        int bi[FAM_MAX_Q];
        // ---- the stage's new medoid: least column sum (q = 1) or greatest gain against the stage before (near[] still holds it)
        bv[0] = inf;
        bi[0] = 0x7fffffff;
        for (int c = t; c < m; c += FAM_THREADS) {
            double s = 0.0;
            if (q == 1) {
#pragma unroll 8
                for (int j = 0; j < m; ++j) s += D[(size_t)j * n + c];
            } else {
#pragma unroll 8
                for (int j = 0; j < m; ++j) s += fmax(near[j] - D[(size_t)j * n + c], 0.0);
                s = -s;                                                // (the greatest gain is the least -gain; -0.0 == 0.0)
            }
            if (s < bv[0] || (s == bv[0] && c < bi[0])) { bv[0] = s; bi[0] = c; }
        }
        reduce(bv, bi, 1);
        if (q > 1 && bv[0] == 0.0) break;                              // fewer than q distinct models (uniform: every thread holds the result)
        if (t == 0) smed[st] = bi[0];
        __syncthreads();

        // ---- alternate
        int it = 0, conv = 0;
        while (true) {
            for (int j = t; j < m; j += FAM_THREADS) {                 // assign: nearest medoid, ties to the one that joined first
                double best = inf, sec = inf;
                int which = 0;
                for (int p = 0; p < q; ++p) {
                    const double d = D[(size_t)smed[p] * n + j];       // (the medoid's row: consecutive j)
                    if (d < best) { sec = best; best = d; which = p; }
                    else if (d < sec) sec = d;
                }
                lab[j] = which;
                near[j] = best;
                label[(size_t)st * n + j] = which;
                nearest[(size_t)st * n + j] = best;
                second[(size_t)st * n + j] = q == 1 ? qnan : sec;
            }
            __syncthreads();
            if (it >= a.max_iter) break;
            ++it;
#pragma unroll
            for (int p = 0; p < FAM_MAX_Q; ++p) { bv[p] = inf; bi[p] = 0x7fffffff; }
            for (int c = t; c < m; c += FAM_THREADS) {                 // update: the member with the least sum over its own family
                const int mine = lab[c];
                double s = 0.0;
#pragma unroll 8
                for (int j = 0; j < m; ++j) {
                    const double d = D[(size_t)j * n + c];
                    s += lab[j] == mine ? d : 0.0;
                }
#pragma unroll
                for (int p = 0; p < FAM_MAX_Q; ++p)
                    if (p == mine && (s < bv[p] || (s == bv[p] && c < bi[p]))) { bv[p] = s; bi[p] = c; }
            }
            reduce(bv, bi, q);
            int changed = 0;
#pragma unroll
            for (int p = 0; p < FAM_MAX_Q; ++p) {
                if (p >= q) continue;
                const int now = bi[p] == 0x7fffffff ? smed[p] : bi[p];    // (a family without a member keeps its medoid)
                changed |= now != smed[p] ? 1 : 0;
                bi[p] = now;
            }
            __syncthreads();                                           // (every thread has read smed)
            if (!changed) { conv = 1; break; }
#pragma unroll
            for (int p = 0; p < FAM_MAX_Q; ++p)
                if (p < q && t == 0) smed[p] = bi[p];
            __syncthreads();
        }
        if (t == 0) {
            for (int p = 0; p < q; ++p) medoid[st * Q + p] = smed[p];
            a.iterations[b * Q + st] = it;
            a.converged[b * Q + st] = (uint8_t)conv;
        }
        found = q;
    }
    if (t == 0) a.n_found[b] = found;
}

}  // namespace ensemble
