// gbp_hitmap.h -- what leaves the device of a block's conductivity-depth hit maps (int32 [B, n_value, n_depth], depth fastest,
// 440 KB per sounding): per-depth statistics for the survey summary, and the maps themselves in run-length form for the results
// containers.  Both are one streaming pass (two for the runs: count, then write) over the maps -- HBM-bound integer work; the torch
// formulation they replace (transpose to float64, cumsum, nonzero over 9e8 cells) took 0.1 s per 8 192 soundings, these take a few ms.
// No reference counterpart: the reference derives the same statistics from its Histogram2D posterior on the host, one sounding at a
// time (classes/statistics/Histogram.py: mean / percentile), and stores the maps dense.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gbp_math.h"

namespace hitmap {

// mean[b, z] = sum_v h (c_v) / max(1, sum_v h) + shift_b,  c_v = ((v + 0.5) / nv) 2 hw - hw, shift_b = log_mean_prior[b] / ln 10;
// pq[b, z] = c_{idx} + shift_b with idx = #{v : cumsum_v / tot < q} clamped to nv - 1, q = 0.05, 0.5, 0.95.
// One workgroup per (sounding, 256 depth cells); thread z walks the value bins: the loads of a wave are 64 consecutive ints.
__global__ __launch_bounds__(256) void k_hitmap_stats(int nv, int nz, const int* __restrict__ hm, const double* __restrict__ log_mean_prior,
                                                       double half_width, double* __restrict__ mean, double* __restrict__ p05,
                                                       double* __restrict__ p50, double* __restrict__ p95)
{
    const int b = blockIdx.x, z = blockIdx.y * 256 + threadIdx.x;
    if (z >= nz) return;
    const int* col = hm + (size_t)b * nv * nz + z;
    const double shift = log_mean_prior[b] / 2.302585092994046;
    const double w = 2.0 * half_width;
    long long tot = 0;
    double wsum = 0.0;
#pragma unroll 10                                  // (ten loads in flight per wave: bound by memory-level parallelism before bytes)
    for (int v = 0; v < nv; ++v) {
        const int h = col[(size_t)v * nz];
        tot += h;
        wsum += (double)h * ((((double)v + 0.5) / (double)nv) * w - half_width);
    }
    const double t = (double)(tot > 1 ? tot : 1);
    long long cum = 0;
    int i05 = 0, i50 = 0, i95 = 0;
#pragma unroll 10
    for (int v = 0; v < nv; ++v) {
        cum += col[(size_t)v * nz];
        const double cdf = (double)cum / t;
        i05 += cdf < 0.05;
        i50 += cdf < 0.5;
        i95 += cdf < 0.95;
    }
    const size_t o = (size_t)b * nz + z;
    auto centre = [&](int i) { return (((double)(i < nv - 1 ? i : nv - 1) + 0.5) / (double)nv) * w - half_width; };
    mean[o] = wsum / t + shift;
    p05[o] = centre(i05) + shift;
    p50[o] = centre(i50) + shift;
    p95[o] = centre(i95) + shift;
}

// Up to 8 quantiles in (0, 1), passed by value (kernel arguments: no device copy).
struct Quantiles {
    double q[8];
    int n;
};

// The per-column moments the line products derive from (python: geobipy_amd/line_products.py), one workgroup per (sounding, 256 depth
// cells) as k_hitmap_stats, thread z walking the value cells of its column twice -- the second pass reads the 256 KB column tile of the
// first from L2:
//   total[b, z] = sum_v c_v (int64);  mean[b, z] = k_hitmap_stats's mean (same expression, same order: the same bits);
//   mode_idx[b, z] = first v of max_v c_v (numpy argmax; an empty column: 0);  s1[b, z] = sum_v c_v ln c_v (0 ln 0 = 0; gbp::log_pos);
//   q_idx[k, b, z] = #{v : cumsum_v / max(total, 1) < q_k} clamped to nv - 1 (mesh/Mesh.py _percentile's searchsorted).
// T is the count type: int for the maps themselves, long long for interval marginals (k_hitmap_intervals), whose counts stay below
// 2^31 n_depth < 2^53, so that every conversion to fp64 is exact and the two instances give the same bits on the same counts.
template <typename T>
__global__ __launch_bounds__(256) void k_hitmap_products(int nv, int nz, const T* __restrict__ hm, const double* __restrict__ log_mean_prior,
                                                          double half_width, Quantiles qs, double* __restrict__ mean, int* __restrict__ mode_idx,
                                                          int* __restrict__ q_idx, long long* __restrict__ total, double* __restrict__ s1)
{
    const int b = blockIdx.x, z = blockIdx.y * 256 + threadIdx.x;
    if (z >= nz) return;
    const T* col = hm + (size_t)b * nv * nz + z;
    const double shift = log_mean_prior[b] / 2.302585092994046;
    const double w = 2.0 * half_width;
    long long tot = 0;
    double wsum = 0.0, slog = 0.0;
    T best = col[0];
    int ibest = 0;
#pragma unroll 10
    for (int v = 0; v < nv; ++v) {
        const T h = col[(size_t)v * nz];
        tot += h;
        wsum += (double)h * ((((double)v + 0.5) / (double)nv) * w - half_width);
        if (h > 0) slog += (double)h * gbp::log_pos((double)h);      // (a branch: a wave whose 64 cells are empty skips the logarithm)
        ibest = h > best ? v : ibest;
        best = h > best ? h : best;
    }
    const double t = (double)(tot > 1 ? tot : 1);
    int iq[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) iq[k] = 0;
    long long cum = 0;
#pragma unroll 10
    for (int v = 0; v < nv; ++v) {
        cum += col[(size_t)v * nz];
        const double cdf = (double)cum / t;
#pragma unroll
        for (int k = 0; k < 8; ++k) iq[k] += (k < qs.n) & (cdf < qs.q[k]);
    }
    const size_t o = (size_t)b * nz + z, plane = (size_t)gridDim.x * nz;
    mean[o] = wsum / t + shift;
    mode_idx[o] = ibest;
    total[o] = tot;
    s1[o] = slog;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < qs.n) q_idx[k * plane + o] = iq[k] < nv - 1 ? iq[k] : nv - 1;
}

// Up to 16 classes in log10 conductivity, passed by value (kernel arguments: no device copy).  scale[k] > 0 is the standard deviation.
constexpr int MAX_CLASSES = 16;
struct Classes {
    double mean[MAX_CLASSES];
    double scale[MAX_CLASSES];
    int n;
};

// Class (lithology) probabilities of every column (Minsley, Foks & Bedrosian 2020; the reference's RectilinearMesh2D._compute_probability
// with log=10 along the value axis), one workgroup per (sounding, 256 depth cells) as k_hitmap_stats, thread z walking its column once:
//   x_v = k_hitmap_stats's centre of value cell v + log_mean_prior[b] / ln 10,  w[v][k] = norm.pdf(x_v, mean_k, scale_k) (scipy's form);
//   S_k = sum_v c_v w[v][k] (v ascending);  prob[b, k, z] = S_k / sum_k' S_k' (0 / 0 = NaN: an empty column, or every term underflows);
//   best[b, z] = the first k of the largest probability (numpy argmax: a NaN wins, an all-NaN column gives 0);
//   best_p[b, z] = its probability.
// The prologue builds the sounding's table w [nv][K] in fp64 in LDS (K nv exps per workgroup, the device libm exp: subnormals kept);
// in the column loop every lane of a wave reads the same table row, a broadcast.  KB is the class bucket (K <= KB): accumulators of
// unused classes cost neither registers nor FMAs beyond the bucket.  A wave whose 64 cells of a value row are all empty skips the row.
template <int KB, typename T>
__global__ __launch_bounds__(256) void k_hitmap_classes(int nv, int nz, const T* __restrict__ hm, const double* __restrict__ log_mean_prior,
                                                         double half_width, Classes cl, double* __restrict__ prob, int* __restrict__ best,
                                                         double* __restrict__ best_p)
{
    extern __shared__ double wt[];                 // [nv][K]
    const int b = blockIdx.x, z = blockIdx.y * 256 + threadIdx.x, K = cl.n;
    const double shift = log_mean_prior[b] / 2.302585092994046;
    const double w = 2.0 * half_width;
    for (int i = threadIdx.x; i < nv * K; i += 256) {
        const int v = i / K, k = i - v * K;
        const double x = ((((double)v + 0.5) / (double)nv) * w - half_width) + shift;
        const double y = (x - cl.mean[k]) / cl.scale[k];
        wt[i] = exp(-y * y / 2.0) / 2.5066282746310002 / cl.scale[k];      // scipy: _norm_pdf((x - loc) / scale) / scale
    }
    __syncthreads();
    if (z >= nz) return;
    const T* col = hm + (size_t)b * nv * nz + z;
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = 0.0;
    auto add = [&](T h, int v) {
        if (h != 0) {
            const double c = (double)h;
            const double* row = wt + v * K;
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (k < KB / 2 || k < K) acc[k] += c * row[k];    // (the lower half of a bucket is always in use: K > KB / 2)
        }
    };
    constexpr int U = 10;                          // ten loads in flight per wave, issued before the rows they feed
    int v0 = 0;
    for (; v0 + U <= nv; v0 += U) {
        T h[U];
#pragma unroll
        for (int u = 0; u < U; ++u) h[u] = col[(size_t)(v0 + u) * nz];
#pragma unroll
        for (int u = 0; u < U; ++u) add(h[u], v0 + u);
    }
    for (; v0 < nv; ++v0) add(col[(size_t)v0 * nz], v0);
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k)
        if (k < KB / 2 || k < K) tot += acc[k];
    const size_t o = (size_t)b * nz + z, plane = (size_t)nz;
    double* pb = prob + (size_t)b * K * nz + z;
    int ib = 0;
    double pbest = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (k < KB / 2 || k < K) {
            const double p = acc[k] / tot;
            pb[k * plane] = p;
            const bool take = k == 0 || (pbest == pbest && (p > pbest || p != p));
            ib = take ? k : ib;
            pbest = take ? p : pbest;
        }
    }
    best[o] = ib;
    best_p[o] = pbest;
}

// Replicate chains: the C hit maps of a sounding (rows s C + c of hm) pooled into one, and per depth cell the agreement of the chains
// (no reference counterpart -- the host statement of the rule is geobipy_amd/replicates.py pool_reference).  One
// workgroup per (sounding, 256 depth cells) as k_hitmap_stats; thread z walks the value cells once, the chains inside: per chain c
//   n_c = sum_v h (int64), a_c = sum_v h x_v, q_c = sum_v (h x_v) x_v, e_c = sum_{h > 0} h ln h    (x_v: k_hitmap_stats's centre, no shift;
//   fp64, v ascending) and, of the pooled cell hp[v] = sum_{c: use} h_c[v] -- written as it is formed --, e_p = sum_{hp > 0} hp ln hp.
// P = {c: use[s, c] != 0 and n_c > 0}, m = |P|:  n_used = m;  chain_mean[s, c, z] = a_c / n_c (NaN outside P);
//   rhat = sqrt(((nbar - 1) / nbar W + Bn) / W), W the mean of the chains' variances max(0, (q_c - a_c m_c) / (n_c - 1)) (0: n_c < 2),
//   Bn = sum_P (m_c - mbar)^2 / (m - 1), nbar = N_P / m  (W == 0: 1 when Bn == 0, else +inf);
//   jsd = max(0, [(ln N_P - e_p / N_P) - sum_P (n_c / N_P)(ln n_c - e_c / n_c)] / ln 2) bits;  both NaN when m < 2.
// CB is the chain bucket (CB / 2 < C <= CB, C = 2: CB = 2): chains beyond C and chains switched off by `use` (uniform over the
// workgroup) cost no loads.  U value rows of every chain are loaded before the rows they feed (10 .. 16 loads in flight per wave).
// A wave whose 64 cells of a value row are empty in every chain skips the logarithms.
template <int CB>
__global__ __launch_bounds__(256) void k_hitmap_pool(int C, int nv, int nz, const int* __restrict__ hm, const int* __restrict__ use,
                                                      double half_width, int* __restrict__ pooled, int* __restrict__ n_used,
                                                      double* __restrict__ chain_mean, double* __restrict__ rhat, double* __restrict__ jsd)
{
    const int s = blockIdx.x, z = blockIdx.y * 256 + threadIdx.x;
    if (z >= nz) return;
    const size_t map = (size_t)nv * nz;
    const int* col = hm + (size_t)s * C * map + z;
    int* out = pooled + (size_t)s * map + z;
    const double w = 2.0 * half_width;
    bool on[CB];
    long long n[CB];
    double a[CB], q[CB], e[CB], ep = 0.0;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        on[c] = (c < CB / 2 || c < C) && use[(size_t)s * C + (c < C ? c : 0)] != 0;
        n[c] = 0;
        a[c] = q[c] = e[c] = 0.0;
    }
    auto add = [&](const int (&h)[CB], int v) {
        const double x = (((double)v + 0.5) / (double)nv) * w - half_width;
        int hp = 0;
#pragma unroll
        for (int c = 0; c < CB; ++c) hp += h[c];
        out[(size_t)v * nz] = hp;
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            if (on[c]) {
                const double hx = (double)h[c] * x;
                n[c] += h[c];
                a[c] += hx;
                q[c] += hx * x;
            }
        }
        if (hp > 0) {                              // (a branch: a wave whose 64 cells are empty in every chain skips the logarithms)
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (on[c] && h[c] > 0) e[c] += (double)h[c] * gbp::log_pos((double)h[c]);
            ep += (double)hp * gbp::log_pos((double)hp);
        }
    };
    constexpr int U = CB == 2 ? 5 : (CB == 4 ? 3 : 2);
    int v0 = 0;
    for (; v0 + U <= nv; v0 += U) {
        int h[U][CB];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < CB; ++c) h[u][c] = on[c] ? col[c * map + (size_t)(v0 + u) * nz] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) add(h[u], v0 + u);
    }
    for (; v0 < nv; ++v0) {
        int h[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) h[c] = on[c] ? col[c * map + (size_t)v0 * nz] : 0;
        add(h, v0);
    }
    // the diagnostics: sums over P in ascending c
    const double nan = __builtin_nan("");
    int m = 0;
    long long NP = 0;
    bool in[CB];
    double mc[CB], sw = 0.0, sm = 0.0;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        in[c] = on[c] && n[c] > 0;
        mc[c] = nan;
        if (in[c]) {
            const double nc = (double)n[c];
            mc[c] = a[c] / nc;
            double s2 = 0.0;
            if (n[c] >= 2) {
                s2 = (q[c] - a[c] * mc[c]) / (double)(n[c] - 1);
                s2 = s2 > 0.0 ? s2 : 0.0;
            }
            sw += s2;
            sm += mc[c];
            NP += n[c];
            ++m;
        }
        if (c < CB / 2 || c < C) chain_mean[((size_t)s * C + c) * nz + z] = mc[c];
    }
    double r = nan, j = nan;
    if (m >= 2) {
        const double md = (double)m, W = sw / md, mbar = sm / md, Nd = (double)NP;
        double sb = 0.0;
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if (in[c]) sb += (mc[c] - mbar) * (mc[c] - mbar);
        const double Bn = sb / (double)(m - 1), nbar = Nd / md;
        if (W == 0.0) r = Bn == 0.0 ? 1.0 : __builtin_inf();
        else r = sqrt(((nbar - 1.0) / nbar * W + Bn) / W);
        double sj = 0.0;
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if (in[c]) {
                const double nc = (double)n[c];
                sj += (nc / Nd) * (gbp::log_pos(nc) - e[c] / nc);
            }
        j = ((gbp::log_pos(Nd) - ep / Nd) - sj) / 0.6931471805599453;
        j = j > 0.0 ? j : 0.0;
    }
    const size_t o = (size_t)s * nz + z;
    n_used[o] = m;
    rhat[o] = r;
    jsd[o] = j;
}

// Runs of a row's flattened cells: a run starts at cell 0 and wherever the count differs from the cell before.
// Pass 1 (WRITE = false): counts[b] = number of runs.  Pass 2 (WRITE = true): start / value at ptr[b] + (rank of the run in the row).
// One workgroup per row walks it in tiles of 1024 cells (4 per thread, coalesced); the ranks inside a tile come from a wave ballot
// and a four-wave prefix in LDS.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_hitmap_runs(long long M, const int* __restrict__ hm, long long* __restrict__ counts,
                                                      const long long* __restrict__ ptr, int* __restrict__ start, int* __restrict__ value)
{
    __shared__ int totals[2][4][4];               // [tile parity][sub-tile][wave]: one barrier per tile
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* row = hm + (size_t)b * M;
    long long base = WRITE ? ptr[b] : 0;          // runs written (or counted) before this tile
    int parity = 0;
    for (long long t0 = 0; t0 < M; t0 += 1024, parity ^= 1) {
        int flags[4], vals[4], before[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {             // sub-tile q: cells t0 + 256 q + thread -- consecutive threads, consecutive cells
            const long long j = t0 + 256 * q + threadIdx.x;
            int f = 0, v = 0;
            if (j < M) {
                v = row[j];
                f = (j == 0) || (v != row[j - 1]);
            }
            flags[q] = f; vals[q] = v;
            const unsigned long long m = __ballot(f);
            before[q] = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) totals[parity][q][wave] = __popcll(m);
        }
        __syncthreads();                          // (the other parity's slots are free again: every thread passed the barrier of the tile before)
        // order of the runs inside the tile: sub-tile major, then wave, then lane
        int rank0 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int lower = 0, all = 0;
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) {
                const int c = totals[parity][q][w2];
                lower += (w2 < wave) ? c : 0;
                all += c;
            }
            if (WRITE && flags[q]) {
                const long long r = base + rank0 + lower + before[q];
                start[r] = (int)(t0 + 256 * q + threadIdx.x);
                value[r] = vals[q];
            }
            rank0 += all;
        }
        base += rank0;
    }
    if (!WRITE && threadIdx.x == 0) counts[b] = base;
}

// Inclusive sum over the 64 lanes of a wave in int64, in the vector ALU alone (DPP: row_shr 1 2 4 8 inside the rows of 16 lanes, then
// row_bcast 15 and 31 across them -- the sequence of LLVM's own wave scan for gfx9); lanes without a source add 0.  Every lane of the
// wave must be active.
template <int CTRL, int ROWS>
__device__ __forceinline__ long long dpp_or_zero(long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(unsigned long long)v, CTRL, ROWS, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)v >> 32), CTRL, ROWS, 0xf, false);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ long long wave_inclusive_sum(long long x)
{
    x += dpp_or_zero<0x111, 0xf>(x);               // row_shr:1
    x += dpp_or_zero<0x112, 0xf>(x);               // row_shr:2
    x += dpp_or_zero<0x114, 0xf>(x);               // row_shr:4
    x += dpp_or_zero<0x118, 0xf>(x);               // row_shr:8
    x += dpp_or_zero<0x142, 0xa>(x);               // row_bcast:15 into rows 1 and 3
    x += dpp_or_zero<0x143, 0xc>(x);               // row_bcast:31 into rows 2 and 3
    return x;
}

__device__ __forceinline__ long long wave_read_lane(long long v, int lane)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// Interval marginals: out[b, v, m] = sum of hm[b, v, z] over the depth cells lo[b, m] <= z < hi[b, m] (int64; the ranges clamped to
// [0, nz], hi <= lo: no cells, 0) -- the reference's Histogram[:, lo:hi].marginalize(axis=1) for M ranges at once, which may overlap
// and differ from sounding to sounding.  One wave per workgroup takes ROWS value rows of one sounding, a row at a time: lane l holds the
// four consecutive cells 256 g + 4 l .. + 3 of group g (ALIGNED: one 16-byte load each, the row read once and coalesced; rows that are
// not 16-byte aligned take four 4-byte loads), sums them, the lane sums are scanned across the wave (wave_inclusive_sum: no LDS), and
// each lane writes the exclusive prefix P of its cells to LDS in int64 (P[z] = sum of the cells before z, P[256 G] = the row's sum).
// Then lane m writes P[hi_m] - P[lo_m], M / 64 coalesced stores.  The next row's loads are issued before the current row is worked on.
// Integer sums: exact in any order.  No atomics, no scratch.  LDS: (256 G + 1) 8 B of prefix + 2 M 4 B of ranges.
constexpr int INTERVAL_ROWS = 32;
template <int G, bool ALIGNED>
__global__ __launch_bounds__(64) void k_hitmap_intervals(int nv, int nz, int M, const int* __restrict__ hm, const int* __restrict__ lo,
                                                         const int* __restrict__ hi, long long* __restrict__ out)
{
    extern __shared__ long long interval_lds[];
    long long* P = interval_lds;                                   // [256 G + 1]
    int* slo = reinterpret_cast<int*>(interval_lds + 256 * G + 1); // [M]
    int* shi = slo + M;                                            // [M]
    const int b = blockIdx.x, lane = threadIdx.x;
    for (int m = lane; m < M; m += 64) {
        int l = lo[(size_t)b * M + m], h = hi[(size_t)b * M + m];
        l = l < 0 ? 0 : (l > nz ? nz : l);
        h = h < 0 ? 0 : (h > nz ? nz : h);
        slo[m] = l;
        shi[m] = h > l ? h : l;                                    // (no cells: P[l] - P[l])
    }
    const int v0 = blockIdx.y * INTERVAL_ROWS, v1 = v0 + INTERVAL_ROWS < nv ? v0 + INTERVAL_ROWS : nv;
    const int* map = hm + (size_t)b * nv * nz;
    auto load = [&](int v, int (&x)[G][4]) {
        const int* row = map + (size_t)v * nz;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int z = 256 * g + 4 * lane;
            if (ALIGNED) {                                         // nz % 4 == 0: a group of four is inside the row or outside it
                int4 q = make_int4(0, 0, 0, 0);
                if (z < nz) q = *reinterpret_cast<const int4*>(row + z);
                x[g][0] = q.x; x[g][1] = q.y; x[g][2] = q.z; x[g][3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[g][j] = z + j < nz ? row[z + j] : 0;
            }
        }
    };
    int cur[G][4] = {}, nxt[G][4] = {};
    if (v0 < v1) load(v0, cur);
    __syncthreads();                                               // (the ranges are in LDS)
    const int lo0 = lane < M ? slo[lane] : 0, hi0 = lane < M ? shi[lane] : 0;
    for (int v = v0; v < v1; ++v) {
        if (v + 1 < v1) load(v + 1, nxt);
        long long base = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long s = (long long)cur[g][0] + cur[g][1] + cur[g][2] + cur[g][3];
            const long long inc = wave_inclusive_sum(s);
            long long p = base + inc - s;                          // exclusive prefix of this lane's first cell
            long long* dst = P + 256 * g + 4 * lane;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dst[j] = p;
                p += cur[g][j];
            }
            base += wave_read_lane(inc, 63);
        }
        if (lane == 0) P[256 * G] = base;
        __syncthreads();                                           // (one wave: the prefix is complete)
        long long* dst = out + ((size_t)b * nv + v) * M;
        if (lane < M) dst[lane] = P[hi0] - P[lo0];
        for (int m = lane + 64; m < M; m += 64) dst[m] = P[shi[m]] - P[slo[m]];
        __syncthreads();                                           // (read before the next row overwrites it)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[g][j] = nxt[g][j];
    }
}

// The value rows of a map in which some lane of the wave has a count, as a bit mask spread over the wave: lane l holds the bits of rows
// 64 l .. 64 l + 63 (4 096 rows at most).  RowWalk hands out the set rows in ascending order; everything here is uniform over the wave
// (the words come through v_readlane), so a walk is a scalar loop.  Every lane of the wave must be active.
constexpr int MIXTURE_MAX_ROWS = 64 * 64;
struct RowWalk {
    long long mask;
    unsigned long long word;
    int wi, nwords;
    __device__ __forceinline__ RowWalk(long long mask_, int nv) : mask(mask_), word(0), wi(-1), nwords((nv + 63) >> 6) {}
    __device__ __forceinline__ int next()                            // the next set row, -1 when there is none
    {
        while (word == 0) {
            if (++wi >= nwords) return -1;
            word = (unsigned long long)wave_read_lane(mask, wi);
        }
        const int bit = __builtin_ctzll(word);
        word &= word - 1;
        return 64 * wi + bit;
    }
};

// Where a lane's mixture fits go: weight / mean / sd [B, Kmax (Kmax + 1) / 2, nz] (stage K in slots K (K - 1) / 2 .. + K),
// loglik / ll_change [B, Kmax, nz], misfit [B, Kmax, 2, nz]; depth fastest.
struct MixtureOut {
    double* weight;
    double* mean;
    double* sd;
    double* loglik;
    double* ll_change;
    double* misfit;
};

// Stage K of the mixture rule for the lane's column (geobipy_amd/mixtures.py mixture_reference is the statement):
// K Gaussians fitted to the binned column by n_iter EM iterations from the quantile start, then one closing pass over all nv cells.
// col: the column (stride nz); rows: the WAVE's non-empty value rows (RowWalk's mask), uniform over the wave, so that a value row is
// one coalesced load and the row loop is a scalar loop; the next row's load is issued before the current row's arithmetic.  Lanes
// whose cell of a row is empty skip the row's arithmetic.  The libm exp / log.
template <int K, typename T>
__device__ __forceinline__ void mixture_stage(const T* __restrict__ col, int nv, int nz, long long rows, double half_width, double Nd,
                                              double m, double V, const int* qi, int n_iter, double reg, bool store, const MixtureOut& o,
                                              size_t b, int z, int Kmax)
{
    const double w2 = 2.0 * half_width, dx = w2 / (double)nv;
    auto centre = [&](int v) { return (((double)v + 0.5) / (double)nv) * w2 - half_width; };
    double wt[K], mu[K], s2[K];
    double ll_prev = 0.0;
    if (K == 1) {
        wt[0] = 1.0;
        mu[0] = m;
        s2[0] = V + reg;
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            wt[j] = 1.0 / (double)K;
            mu[j] = centre(qi[j]);
            s2[j] = V / (double)(K * K) + reg;
        }
        for (int it = 0; it < n_iter; ++it) {
            double a[K], h[K], sn[K], sa[K], sq[K], sl = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                a[j] = log(wt[j]) - 0.5 * log(6.283185307179586 * s2[j]);
                h[j] = 2.0 * s2[j];
                sn[j] = sa[j] = sq[j] = 0.0;
            }
            RowWalk walk(rows, nv);
            int v = walk.next();
            T cn = v >= 0 ? col[(size_t)v * nz] : (T)0;
            while (v >= 0) {
                const int vn = walk.next();
                const T ci = cn;
                if (vn >= 0) cn = col[(size_t)vn * nz];
                if (ci > 0) {
                    const double c = (double)ci, x = centre(v);
                    double d[K], l[K], top;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        d[j] = x - mu[j];
                        l[j] = a[j] - d[j] * d[j] / h[j];
                    }
                    top = l[0];
#pragma unroll
                    for (int j = 1; j < K; ++j) top = l[j] > top ? l[j] : top;
                    double se = 0.0;
#pragma unroll
                    for (int j = 0; j < K; ++j) se += exp(l[j] - top);
                    const double L = top + log(se);
                    sl += c * L;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const double r = c * exp(l[j] - L);
                        sn[j] += r;
                        sa[j] += r * d[j];
                        sq[j] += r * d[j] * d[j];
                    }
                }
                v = vn;
            }
            double nt = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                sn[j] += 10.0 * 2.220446049250313e-16;
                nt += sn[j];
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double g = sa[j] / sn[j];
                const double var = sq[j] / sn[j] - g * g;
                mu[j] += g;
                s2[j] = (var > 0.0 ? var : 0.0) + reg;
                wt[j] = sn[j] / nt;
            }
            ll_prev = sl / Nd;
        }
    }
    // the closing pass: every cell of the column
    double a[K], h[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        a[j] = log(wt[j]) - 0.5 * log(6.283185307179586 * s2[j]);
        h[j] = 2.0 * s2[j];
    }
    double sl = 0.0, emax = 0.0, pmax = 0.0, e2 = 0.0, p2 = 0.0;
    T cn = col[0];
    for (int v = 0; v < nv; ++v) {
        const T ci = cn;
        if (v + 1 < nv) cn = col[(size_t)(v + 1) * nz];
        const double c = (double)ci, x = centre(v);
        double l[K], top;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double d = x - mu[j];
            l[j] = a[j] - d * d / h[j];
        }
        top = l[0];
#pragma unroll
        for (int j = 1; j < K; ++j) top = l[j] > top ? l[j] : top;
        double se = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) se += exp(l[j] - top);
        const double L = top + log(se);
        sl += c * L;
        const double p = c / Nd, e = fabs(p - exp(L) * dx);
        emax = e > emax ? e : emax;
        pmax = p > pmax ? p : pmax;
        e2 += e * e;
        p2 += p * p;
    }
    if (!store) return;
    const double nan = __builtin_nan("");
    const bool some = Nd > 0.0;
    const double loglik = sl / Nd;
    const size_t S = (size_t)(Kmax * (Kmax + 1) / 2), slot = (size_t)(K * (K - 1) / 2);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const size_t i = (b * S + slot + j) * nz + z;
        o.weight[i] = some ? wt[j] : nan;
        o.mean[i] = some ? mu[j] : nan;
        o.sd[i] = some ? sqrt(s2[j]) : nan;
    }
    const size_t i = (b * Kmax + (K - 1)) * nz + z;
    o.loglik[i] = some ? loglik : nan;
    o.ll_change[i] = some ? (K == 1 ? 0.0 : loglik - ll_prev) : nan;
    o.misfit[(2 * (b * Kmax + (K - 1)) + 0) * nz + z] = some ? emax / pmax : nan;
    o.misfit[(2 * (b * Kmax + (K - 1)) + 1) * nz + z] = some ? sqrt(e2) / sqrt(p2) : nan;
}

// Local mixture fits: all stages K = 1 .. Kmax of every (sounding, depth cell) column in one launch, one workgroup
// per (sounding, 256 depth cells) and one lane per column as k_hitmap_stats.  Pass 1 walks the column: N (int64), sum c x, and the
// wave's non-empty rows (a ballot per row; RowWalk's mask).  Pass 2 walks those rows: V = sum c (x - m)^2 / N and, for every stage
// and component, the quantile start cell, the first v with 2 K cum_v >= (2 j + 1) N (int64, exact: the row at which the lane's
// cumulative count crosses).  Then the stages (mixture_stage), whose EM passes walk the non-empty rows only.  The rows are re-read
// from L1 / L2 in every pass (a wave's 10 .. 40 rows are 2.5 .. 10 KB; the arithmetic per row -- K exp, a log, K exp again -- outweighs
// the load by two orders): no LDS.  Lanes beyond nz repeat the last column and store nothing, so that every lane of a wave takes part
// in the ballots.  nv <= MIXTURE_MAX_ROWS.
template <typename T>
__global__ __launch_bounds__(256) void k_hitmap_mixture(int nv, int nz, const T* __restrict__ hm, double half_width, int Kmax, int n_iter,
                                                         double reg, MixtureOut o)
{
    const int b = blockIdx.x, z = blockIdx.y * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool store = z < nz;
    const int zc = store ? z : nz - 1;
    const T* col = hm + (size_t)b * nv * nz + zc;
    const double w2 = 2.0 * half_width;
    long long tot = 0, rows = 0;
    double wsum = 0.0;
    auto add = [&](T h, int v) {
        tot += h;
        wsum += (double)h * ((((double)v + 0.5) / (double)nv) * w2 - half_width);
        if (__ballot(h > 0) != 0 && lane == (v >> 6)) rows |= 1ll << (v & 63);
    };
    constexpr int U = 10;                          // ten loads in flight per wave, issued before the rows they feed
    int v0 = 0;
    for (; v0 + U <= nv; v0 += U) {
        T h[U];
#pragma unroll
        for (int u = 0; u < U; ++u) h[u] = col[(size_t)(v0 + u) * nz];
#pragma unroll
        for (int u = 0; u < U; ++u) add(h[u], v0 + u);
    }
    for (; v0 < nv; ++v0) add(col[(size_t)v0 * nz], v0);
    const double Nd = (double)tot, m = wsum / Nd;
    // quantile start cells: stage K = 2 .. 4 at qi[K (K - 1) / 2 - 1 + j]
    int qi[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) qi[i] = 0;
    long long cum = 0;
    double vsum = 0.0;
    RowWalk walk(rows, nv);
    for (int v = walk.next(); v >= 0; v = walk.next()) {
        const T h = col[(size_t)v * nz];
        const double d = ((((double)v + 0.5) / (double)nv) * w2 - half_width) - m;
        vsum += (double)h * d * d;
        const long long before = cum;
        cum += h;
#pragma unroll
        for (int K = 2; K <= 4; ++K)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const long long t = (2 * j + 1) * tot;
                qi[K * (K - 1) / 2 - 1 + j] = (2 * K * before < t && 2 * K * cum >= t) ? v : qi[K * (K - 1) / 2 - 1 + j];
            }
    }
    const double V = vsum / Nd;
    mixture_stage<1, T>(col, nv, nz, rows, half_width, Nd, m, V, qi, n_iter, reg, store, o, (size_t)b, z, Kmax);
    if (Kmax >= 2) mixture_stage<2, T>(col, nv, nz, rows, half_width, Nd, m, V, qi + 0, n_iter, reg, store, o, (size_t)b, z, Kmax);
    if (Kmax >= 3) mixture_stage<3, T>(col, nv, nz, rows, half_width, Nd, m, V, qi + 2, n_iter, reg, store, o, (size_t)b, z, Kmax);
    if (Kmax >= 4) mixture_stage<4, T>(col, nv, nz, rows, half_width, Nd, m, V, qi + 5, n_iter, reg, store, o, (size_t)b, z, Kmax);
}

}  // namespace hitmap
