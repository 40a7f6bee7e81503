// Sections across flight lines (geobipy_amd/sections.py propagate_reference states the rule in numpy;
// include/geobipy_amd.h gbp_section_propagate): synchronous sum-product message passing (loopy belief propagation) on the survey graph.
// The states of sounding s are its m_s = n_used[s] of n <= 256 kept models with weights w_s = exp(score_s); the undirected edge
// e = {u, v}, u < v, carries K_e[i, j] = exp(-(g[e] * d2[e, i, j])), i a state of u and j a state of v.  Directed edge 2 e is u -> v
// (through K_e), 2 e + 1 is v -> u (through its transpose); a message mu[d] has m_dst entries and starts at 1 / m_dst.
//
//   k_graph_kernel   d2 -> K, one multiply and one exp per entry of the prefix i < m_u, j < m_v; streaming, one workgroup per edge.
//   k_graph_init     w = exp(score) [S, n] and the first messages [2 E, n].
//   k_graph_sweep    one launch per sweep, one 256-thread workgroup per UNDIRECTED edge: K_e is read from memory once and serves both
//                    directions.  h_u (all of u's incoming messages but v's, times w_u) and h_v are built in LDS through the CSR of
//                    incoming directed edges (in_ptr [S + 1], in_edge sorted by neighbour), in the rule's order.  K_e passes through LDS
//                    in tiles of 64 x 64 doubles with a leading dimension of 65 (33 280 B): the four waves fetch a tile with reads that
//                    are coalesced along j; wave 0 walks its columns (lane = j, i ascending: u -> v), wave 1 its rows (lane = i, j
//                    ascending: v -> u).  A column read is 64 consecutive doubles and a row read has a stride of 65 doubles = 130 banks,
//                    2 l mod 64 over the 32 lanes of a ds_read_b64 group: both are free of bank conflicts, and neither direction reads
//                    global memory with a stride of n.  Tiles run ti outer, tj inner; the column sums live in LDS across ti, the row
//                    sums in a register across tj, so every sum adds its terms in ascending order of the source state whatever n is:
//                    the operations of the rule, one multiply and one add per term (-ffp-contract=off).  tot is summed by one lane per
//                    direction, in the rule's order.  LDS per workgroup: the tile and four vectors of MAXN doubles, 35 408 B for
//                    n <= 64 (MAXN = 64: 4 workgroups, 16 waves, per CU of 160 KiB) and 41 552 B for n <= 256 (3 workgroups); the
//                    registers allow 5 waves per SIMD, so LDS sets the occupancy.
//   k_graph_residual the largest of the [2 E] per-message residuals of every sweep, in a fixed order; a NaN stays.
//   k_graph_belief   one workgroup per sounding: w_s times all incoming messages (ascending neighbour), divided by its sum (one lane, i
//                    ascending), and the first maximum.
// No atomics, and no sum whose order depends on scheduling: a call repeats its own bits.  Nothing outside the prefixes of d2 is read.
// An index that does not fit (an endpoint outside 0 .. S - 1, an entry of in_edge outside 0 .. 2 E - 1) is skipped, never followed.
#pragma once

#include "gbp_section.h"

namespace section {

constexpr int GRAPH_MAX_STATES = 256, GRAPH_TILE = 64, GRAPH_LD = GRAPH_TILE + 1;

// max that keeps a NaN once it has one (fmax would drop it): the residual of a sweep with a NaN message is NaN, as numpy's max is.
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double wave_nan_max(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(THREADS) void k_graph_kernel(int S, int n, const int* __restrict__ eu, const int* __restrict__ ev,
                                                          const int* __restrict__ n_used, const double* __restrict__ g,
                                                          const double* __restrict__ d2, double* __restrict__ K)
{
    const size_t e = blockIdx.x;
    const int u = eu[e], v = ev[e];
    if (u < 0 || u >= S || v < 0 || v >= S) return;
    const int mu = used(n_used, (size_t)u, n), mv = used(n_used, (size_t)v, n);
    const double ge = g[e];
    const double* const D = d2 + e * (size_t)n * n;
    double* const Ke = K + e * (size_t)n * n;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int i = wave; i < mu; i += WAVES)
        for (int j = lane; j < mv; j += 64) Ke[(size_t)i * n + j] = exp(-(ge * D[(size_t)i * n + j]));
}

// w [S, n] = exp(score) on the prefix, 0.0 beyond; both message buffers [2 E, n] = 1 / m_dst on the prefix, 0.0 beyond.  Block b < S is
// a sounding, block S + d a directed edge.
__global__ __launch_bounds__(THREADS) void k_graph_init(int S, int E, int n, const int* __restrict__ eu, const int* __restrict__ ev,
                                                        const int* __restrict__ n_used, const double* __restrict__ score,
                                                        double* __restrict__ w, double* __restrict__ mu0, double* __restrict__ mu1)
{
    const int t = (int)threadIdx.x;
    if ((int)blockIdx.x < S) {
        const size_t s = blockIdx.x;
        const int m = used(n_used, s, n);
        if (t < n) w[s * n + t] = t < m ? exp(score[s * n + t]) : 0.0;
        return;
    }
    const size_t d = (size_t)blockIdx.x - (size_t)S;
    const int dst = (d & 1) ? eu[d >> 1] : ev[d >> 1];
    if (t >= n) return;
    double first = 0.0;
    if (dst >= 0 && dst < S) {
        const int m = used(n_used, (size_t)dst, n);
        first = t < m ? 1.0 / (double)m : 0.0;
    }
    mu0[d * n + t] = first;
    mu1[d * n + t] = first;
}

// w_a[t] times the messages into a, in_edge order (ascending neighbour), but the one of directed edge `skip`.
__device__ __forceinline__ double graph_h(int a, int t, int n, long long twoE, long long skip, const double* __restrict__ w,
                                          const int* __restrict__ in_ptr, const int* __restrict__ in_edge, const double* __restrict__ mu)
{
    double h = w[(size_t)a * n + t];
    const int q1 = (int)min((long long)in_ptr[a + 1], twoE);
    for (int q = max(in_ptr[a], 0); q < q1; ++q) {
        const long long d = in_edge[q];
        if (d != skip && d >= 0 && d < twoE) h = h * mu[(size_t)d * n + t];
    }
    return h;
}

template <bool DAMP, int MAXN>
__global__ __launch_bounds__(THREADS) void k_graph_sweep(int S, int E, int n, const int* __restrict__ eu, const int* __restrict__ ev,
                                                         const int* __restrict__ n_used, const double* __restrict__ w,
                                                         const double* __restrict__ K, const int* __restrict__ in_ptr,
                                                         const int* __restrict__ in_edge, const double* __restrict__ mu_old,
                                                         double* __restrict__ mu_new, double damping, double* __restrict__ resid)
{
    __shared__ double tile[GRAPH_TILE * GRAPH_LD];
    __shared__ double hu[MAXN], hv[MAXN], au[MAXN], av[MAXN];               // n <= MAXN: 64 or 256
    __shared__ double red[2 * WAVES], tot[2];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t e = blockIdx.x;
    const long long twoE = 2 * (long long)E, d_uv = 2 * (long long)e, d_vu = d_uv + 1;
    const int u = eu[e], v = ev[e];
    if (u < 0 || u >= S || v < 0 || v >= S) {                               // (not an edge of this graph: its messages keep their values)
        if (t < 2) resid[d_uv + t] = 0.0;
        return;
    }
    const int mu = used(n_used, (size_t)u, n), mv = used(n_used, (size_t)v, n);
    if (t < mu) hu[t] = graph_h(u, t, n, twoE, d_vu, w, in_ptr, in_edge, mu_old);
    if (t < mv) {
        hv[t] = graph_h(v, t, n, twoE, d_uv, w, in_ptr, in_edge, mu_old);
        av[t] = 0.0;
    }
    const int TI = (mu + GRAPH_TILE - 1) / GRAPH_TILE, TJ = (mv + GRAPH_TILE - 1) / GRAPH_TILE;
    const double* const Ke = K + e * (size_t)n * n;
    for (int ti = 0; ti < TI; ++ti) {
        const int i0 = ti * GRAPH_TILE, ni = min(GRAPH_TILE, mu - i0);
        double row = 0.0;                                                   // wave 1: the sum of row i0 + lane over the tiles so far
        for (int tj = 0; tj < TJ; ++tj) {
            const int j0 = tj * GRAPH_TILE, nj = min(GRAPH_TILE, mv - j0);
            __syncthreads();                                                // h is whole; the last tile's readers are done
            if (lane < nj) {
#pragma unroll
                for (int k = 0; k < GRAPH_TILE / WAVES; ++k) {
                    const int ii = wave + WAVES * k;
                    if (ii < ni) tile[ii * GRAPH_LD + lane] = Ke[(size_t)(i0 + ii) * n + j0 + lane];
                }
            }
            __syncthreads();
            if (wave == 0) {                                                // u -> v: down column j0 + lane
                if (lane < nj) {
                    double a = av[j0 + lane];
#pragma unroll 8
                    for (int ii = 0; ii < ni; ++ii) a = a + hu[i0 + ii] * tile[ii * GRAPH_LD + lane];
                    av[j0 + lane] = a;
                }
            } else if (wave == 1) {                                         // v -> u: along row i0 + lane
                if (lane < ni) {
#pragma unroll 8
                    for (int jj = 0; jj < nj; ++jj) row = row + hv[j0 + jj] * tile[lane * GRAPH_LD + jj];
                }
            }
        }
        if (wave == 1 && lane < ni) au[i0 + lane] = row;
    }
    __syncthreads();
    if (t == 0) {                                                           // the rule's order: one lane, ascending
        double s = 0.0;
        for (int j = 0; j < mv; ++j) s = s + av[j];
        tot[0] = s;
    } else if (t == 64) {
        double s = 0.0;
        for (int i = 0; i < mu; ++i) s = s + au[i];
        tot[1] = s;
    }
    __syncthreads();
    double r_uv = 0.0, r_vu = 0.0;
    if (t < mv) {
        const double old = mu_old[(size_t)d_uv * n + t];
        double m = av[t] / tot[0];
        if (DAMP) m = (1.0 - damping) * m + damping * old;
        mu_new[(size_t)d_uv * n + t] = m;
        r_uv = fabs(m - old);
    }
    if (t < mu) {
        const double old = mu_old[(size_t)d_vu * n + t];
        double m = au[t] / tot[1];
        if (DAMP) m = (1.0 - damping) * m + damping * old;
        mu_new[(size_t)d_vu * n + t] = m;
        r_vu = fabs(m - old);
    }
    r_uv = wave_nan_max(r_uv);
    r_vu = wave_nan_max(r_vu);
    if (lane == 0) {
        red[wave] = r_uv;
        red[WAVES + wave] = r_vu;
    }
    __syncthreads();
    if (t < 2) resid[d_uv + t] = nan_max(nan_max(nan_max(red[WAVES * t], red[WAVES * t + 1]), red[WAVES * t + 2]), red[WAVES * t + 3]);
}

// residual[s] = the largest of resid[s, 0 .. 2 E - 1] (0.0 without edges); one workgroup per sweep.
__global__ __launch_bounds__(THREADS) void k_graph_residual(long long twoE, const double* __restrict__ resid, double* __restrict__ residual)
{
    __shared__ double red[WAVES];
    const int t = (int)threadIdx.x;
    const double* const R = resid + (size_t)blockIdx.x * (size_t)twoE;
    double r = 0.0;
    for (long long d = t; d < twoE; d += THREADS) r = nan_max(r, R[d]);
    r = wave_nan_max(r);
    if ((t & 63) == 0) red[t >> 6] = r;
    __syncthreads();
    if (t == 0) residual[blockIdx.x] = nan_max(nan_max(nan_max(red[0], red[1]), red[2]), red[3]);
}

__global__ __launch_bounds__(THREADS) void k_graph_belief(int E, int n, const int* __restrict__ n_used, const double* __restrict__ w,
                                                          const int* __restrict__ in_ptr, const int* __restrict__ in_edge,
                                                          const double* __restrict__ mu, double* __restrict__ belief, int* __restrict__ state)
{
    __shared__ double h[GRAPH_MAX_STATES];
    __shared__ double tot;
    const int t = (int)threadIdx.x;
    const size_t s = blockIdx.x;
    const int m = used(n_used, s, n);
    if (t < m) h[t] = graph_h((int)s, t, n, 2 * (long long)E, -1, w, in_ptr, in_edge, mu);
    __syncthreads();
    if (t == 0) {
        double a = 0.0;
        for (int i = 0; i < m; ++i) a = a + h[i];
        tot = a;
    }
    __syncthreads();
    if (t < m) h[t] = h[t] / tot;
    if (t < n) belief[s * n + t] = t < m ? h[t] : 0.0;
    __syncthreads();
    if (t == 0) {                                                           // the first maximum: strict >, a NaN never replaces
        int cur = 0;
        double top = h[0];
        for (int i = 1; i < m; ++i)
            if (h[i] > top) {
                top = h[i];
                cur = i;
            }
        state[s] = cur;
    }
}

}  // namespace section
