// The evidence of the lateral coupling along lines (geobipy_amd/sections.py evidence_reference states the rule in
// numpy; include/geobipy_amd.h gbp_section_evidence): log Z of the chain of gbp_section.h and its derivative in lambda = ln c for a
// ladder of scales c_t = c_0 2^t of the step costs, from ONE forward pass over d2.
//
//   k_section_evidence<NJ, T>  one 256-thread workgroup walks one sequence, as k_section_viterbi does: thread t owns the columns
//                              (t mod W) + 256 jj and walks i upward over column j of d2[r].  Per entry it takes one multiply (cost_0 =
//                              g[r] d2[r, i, j]) and ONE exp (e_0 = exp(-cost_0)); rung t + 1 is e * e and cost + cost, which is exact for
//                              the cost and costs the weight one rounding per squaring.  Per column and rung it carries two fp64 sums in
//                              registers: u = sum_i a_t[i] e_t and u' = sum_i (b_t[i] - a_t[i] cost_t) e_t, a_t the normalised filter of
//                              rung t and b_t = d a_t / d lambda its tangent.  (a_t, b_t) lie in LDS as pairs, double-buffered: one
//                              16-byte broadcast read per rung and row.  With n <= 128 the G = 256 / W lane groups (W = 64, 128 or 256
//                              >= n) each take a contiguous part of the i range and meet in LDS, the lower part first.  ROWS rows of
//                              d2 are on their way while the rows before them are worked on; the next step's g and n_used are asked for
//                              a step ahead.
//   k_graph_evidence           the same for the survey graph, through the Bethe free energy of the messages gbp_section_propagate
//                              leaves: a workgroup per edge and one per sounding; see the kernel (include/geobipy_amd.h
//                              gbp_section_graph_evidence; sections.graph_terms_reference states the rule).
// Nothing outside the prefixes i < m_r, j < m_{r+1} is read.  No workspace in memory, no backward pass, no atomics: a call repeats its
// bits.  The sums over i and j are not in numpy's order: the device is held to the rule within a bound, not to bits.
#pragma once

#include "gbp_section.h"
#include "gbp_section_graph.h"

namespace section {

constexpr int EVIDENCE_MAX_RUNGS = 8, EVIDENCE_MAX_STATES = 2048;           // T, and T * n: the pairs (a_t, b_t) twice in LDS are 64 KiB

inline int evidence_width(int n) { return n <= 64 ? 64 : n <= 128 ? 128 : THREADS; }

// the pairs [2, T, n], the partial sums of the waves [2 T, WAVES] and, where lane groups meet, theirs [2 T, THREADS]
inline size_t evidence_lds_bytes(int n, int T)
{
    return ((size_t)4 * T * n + (size_t)2 * T * WAVES + (evidence_width(n) < THREADS ? (size_t)2 * T * THREADS : 0)) * sizeof(double);
}

// The sums of v[0 .. K - 1] over the workgroup, the same in every thread: lanes by butterfly, then the four waves in order.  red
// [K, WAVES] must be free on entry (the caller's last barrier) and is read until the caller's next one.
template <int K>
__device__ __forceinline__ void evidence_sums(double (&v)[K], double* red)
{
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[k * WAVES + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k * WAVES] + red[k * WAVES + 1]) + red[k * WAVES + 2]) + red[k * WAVES + 3];
}

template <int NJ, int T>
__global__ __launch_bounds__(THREADS) void k_section_evidence(const long long* __restrict__ ptr, int L, int n, int W,
                                                              const int* __restrict__ n_used, const double* __restrict__ score,
                                                              const double* __restrict__ g, const double* __restrict__ d2,
                                                              double* __restrict__ log_partition, double* __restrict__ dlog_partition)
{
    constexpr int ROWS = NJ == 1 ? 16 : NJ == 2 ? 8 : 4;                    // rows of d2 a lane has on their way: 16 doubles in every instance
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = (int)threadIdx.x, G = THREADS / W, col = t & (W - 1), part = t / W;
    double2* const AB = (double2*)lds;                                      // (a_t[i], b_t[i]) at [buffer, t, i]
    double* const red = lds + (size_t)4 * T * n;
    double* const parts = red + 2 * T * WAVES;
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) {
        if (t == 0)
            for (int k = 0; k < T; ++k) log_partition[(size_t)k * L + blockIdx.x] = dlog_partition[(size_t)k * L + blockIdx.x] = 0.0;
        return;
    }
    int m = used(n_used, (size_t)r0, n);
    double lz[T], dlz[T];
    {
        double w0[NJ], s[1] = {0.0};
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = col + THREADS * jj;
            w0[jj] = part == 0 && j < m ? exp(score[(size_t)r0 * n + j]) : 0.0;
            s[0] += w0[jj];
        }
        evidence_sums<1>(s, red);
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = col + THREADS * jj;
            if (part == 0 && j < m) {
                const double2 ab = make_double2(w0[jj] / s[0], 0.0);
#pragma unroll
                for (int k = 0; k < T; ++k) AB[(size_t)k * n + j] = ab;
            }
        }
        const double l0 = log(s[0]);
#pragma unroll
        for (int k = 0; k < T; ++k) {
            lz[k] = l0;
            dlz[k] = 0.0;
        }
    }
    __syncthreads();                                                        // the first filter is whole; red is free
    int cur = 0;
    int mn = N > 1 ? used(n_used, (size_t)r0 + 1, n) : 1;
    double gr = g[r0];
    for (int st = 0; st + 1 < N; ++st) {
        const size_t r = (size_t)r0 + st;
        const int m_after = st + 2 < N ? used(n_used, r + 2, n) : 1;        // the next step's, asked for a step ahead: nobody waits for them
        const double g_next = g[r + 1];
        const int chunk = (m + G - 1) / G, i0 = part * chunk, i1 = min(m, i0 + chunk);
        const double* const D = d2 + r * (size_t)n * n;
        const double2* const A = AB + (size_t)cur * T * n;
        int jc[NJ];
        double wn[NJ], u[NJ][T], up[NJ][T];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            jc[jj] = min(col + THREADS * jj, mn - 1);                       // (a lane without a state walks the last column: no read outside the prefix)
            wn[jj] = score[(r + 1) * n + jc[jj]];
#pragma unroll
            for (int k = 0; k < T; ++k) u[jj][k] = up[jj][k] = 0.0;
        }
        double ahead[ROWS][NJ];                                             // rows i .. i + ROWS - 1, capped at the prefix's last row
#pragma unroll
        for (int q = 0; q < ROWS; ++q)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) ahead[q][jj] = D[(size_t)min(i0 + q, m - 1) * n + jc[jj]];
        for (int i = i0; i < i1; i += ROWS) {
            double now[ROWS][NJ];
#pragma unroll
            for (int q = 0; q < ROWS; ++q)
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj) {
                    now[q][jj] = ahead[q][jj];
                    ahead[q][jj] = D[(size_t)min(i + ROWS + q, m - 1) * n + jc[jj]];
                }
#pragma unroll
            for (int q = 0; q < ROWS; ++q) {
                if (i + q < i1) {                                           // (the same in every lane of a wave: W >= 64)
                    double2 ab[T];
#pragma unroll
                    for (int k = 0; k < T; ++k) ab[k] = A[(size_t)k * n + i + q];
#pragma unroll
                    for (int jj = 0; jj < NJ; ++jj) {
                        double cost = gr * now[q][jj];
                        double e = exp(-cost);
#pragma unroll
                        for (int k = 0; k < T; ++k) {
                            u[jj][k] = u[jj][k] + ab[k].x * e;
                            up[jj][k] = up[jj][k] + (ab[k].y - ab[k].x * cost) * e;
                            e = e * e;
                            cost = cost + cost;
                        }
                    }
                }
            }
        }
        if (G > 1) {                                                        // (NJ == 1: the lane groups meet, the lower part of i first)
#pragma unroll
            for (int k = 0; k < T; ++k) {
                parts[(2 * k) * THREADS + t] = u[0][k];
                parts[(2 * k + 1) * THREADS + t] = up[0][k];
            }
            __syncthreads();
            if (part == 0)
                for (int p = 1; p < G; ++p) {
#pragma unroll
                    for (int k = 0; k < T; ++k) {
                        u[0][k] = u[0][k] + parts[(2 * k) * THREADS + p * W + col];
                        up[0][k] = up[0][k] + parts[(2 * k + 1) * THREADS + p * W + col];
                    }
                }
        }
        double z[2 * T];
#pragma unroll
        for (int k = 0; k < T; ++k) z[2 * k] = z[2 * k + 1] = 0.0;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const bool live = part == 0 && col + THREADS * jj < mn;
            const double w = exp(wn[jj]);
#pragma unroll
            for (int k = 0; k < T; ++k) {
                u[jj][k] = live ? w * u[jj][k] : 0.0;
                up[jj][k] = live ? w * up[jj][k] : 0.0;
                z[2 * k] += u[jj][k];
                z[2 * k + 1] += up[jj][k];
            }
        }
        evidence_sums<2 * T>(z, red);
        double2* const An = AB + (size_t)(cur ^ 1) * T * n;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const double ratio = z[2 * k + 1] / z[2 * k];
            lz[k] += log(z[2 * k]);
            dlz[k] += ratio;
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int j = col + THREADS * jj;
                if (part == 0 && j < mn) {
                    const double a = u[jj][k] / z[2 * k];
                    An[(size_t)k * n + j] = make_double2(a, up[jj][k] / z[2 * k] - a * ratio);
                }
            }
        }
        __syncthreads();                                                    // the next filter is whole; this one, red and the parts are free
        cur ^= 1;
        m = mn;
        mn = m_after;
        gr = g_next;
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < T; ++k) {
            log_partition[(size_t)k * L + blockIdx.x] = lz[k];
            dlog_partition[(size_t)k * L + blockIdx.x] = dlz[k];
        }
    }
}

// The terms of the Bethe evidence of the survey graph from the messages of gbp_section_propagate (sections.graph_terms_reference states
// the rule).  Block e < E is an undirected edge {u, v}: h_u = w_u times the messages into u but v's, h_v likewise, built in LDS through
// the CSR as k_graph_sweep builds them; the edge's d2 is streamed once, wave by row and lane by column, K = exp(-(g[e] * d2)):
// edge_log_z[e] = ln sum_ij h_u[i] K_ij h_v[j] and edge_energy[e] = g[e] sum_ij h_u[i] K_ij d2_ij h_v[j] / that sum, the expected
// cost of the edge under its own belief.  Block E + s is a sounding: node_log_z[s] = ln sum_i w_s[i] times all its incoming messages.
// Sums by lane, butterfly and wave in a fixed order: a call repeats its bits.  An edge whose endpoints do not fit gets 0.0 and 0.0.
__global__ __launch_bounds__(THREADS) void k_graph_evidence(int S, int E, int n, const int* __restrict__ eu, const int* __restrict__ ev,
                                                            const int* __restrict__ n_used, const double* __restrict__ w,
                                                            const double* __restrict__ g, const double* __restrict__ d2,
                                                            const int* __restrict__ in_ptr, const int* __restrict__ in_edge,
                                                            const double* __restrict__ mu, double* __restrict__ node_log_z,
                                                            double* __restrict__ edge_log_z, double* __restrict__ edge_energy)
{
    __shared__ double hu[GRAPH_MAX_STATES], hv[GRAPH_MAX_STATES];
    __shared__ double red[2 * WAVES];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long twoE = 2 * (long long)E;
    if ((int)blockIdx.x >= E) {
        const int s = (int)blockIdx.x - E;
        const int m = used(n_used, (size_t)s, n);
        double tot[1] = {t < m ? graph_h(s, t, n, twoE, -1, w, in_ptr, in_edge, mu) : 0.0};
        evidence_sums<1>(tot, red);
        if (t == 0) node_log_z[s] = log(tot[0]);
        return;
    }
    const size_t e = blockIdx.x;
    const long long d_uv = 2 * (long long)e, d_vu = d_uv + 1;
    const int u = eu[e], v = ev[e];
    if (u < 0 || u >= S || v < 0 || v >= S) {                               // (not an edge of this graph)
        if (t == 0) edge_log_z[e] = edge_energy[e] = 0.0;
        return;
    }
    const int m_u = used(n_used, (size_t)u, n), m_v = used(n_used, (size_t)v, n);
    if (t < m_u) hu[t] = graph_h(u, t, n, twoE, d_vu, w, in_ptr, in_edge, mu);
    if (t < m_v) hv[t] = graph_h(v, t, n, twoE, d_uv, w, in_ptr, in_edge, mu);
    __syncthreads();
    const double ge = g[e];
    const double* const D = d2 + e * (size_t)n * n;
    double acc[2] = {0.0, 0.0};
    for (int i = wave; i < m_u; i += WAVES) {
        double rz = 0.0, re = 0.0;
        for (int j = lane; j < m_v; j += 64) {
            const double d = D[(size_t)i * n + j];
            const double p = exp(-(ge * d)) * hv[j];
            rz = rz + p;
            re = re + p * d;
        }
        acc[0] = acc[0] + hu[i] * rz;
        acc[1] = acc[1] + hu[i] * re;
    }
    evidence_sums<2>(acc, red);
    if (t == 0) {
        edge_log_z[e] = log(acc[0]);
        edge_energy[e] = ge * acc[1] / acc[0];
    }
}

}  // namespace section
