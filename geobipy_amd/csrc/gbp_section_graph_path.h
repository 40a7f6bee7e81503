// The most probable section across flight lines (geobipy_amd/sections.py graph_path_reference states the rule in numpy;
// include/geobipy_amd.h gbp_section_graph_path, gbp_section_graph_refine): synchronous max-sum message passing on the survey graph of
// gbp_section_graph.h, a decode by conditioning level by level, and coordinate ascent on the exact score.  Everything is in the log
// domain: theta_s = score[s], the edge e = {u, v}, u < v, costs c_e[i, j] = g[e] * d2[e, i, j], a message nu[d] has m_dst entries and
// starts at 0.0.  There is no exp and no sum whose order could differ from the rule's: the device has the rule's bits.
//
//   k_graph_maxsum       one launch per sweep, one 256-thread workgroup per UNDIRECTED edge, on the plan of k_graph_sweep: h_u and h_v
//                        (theta plus all incoming messages but the partner's, the rule's order) are built in LDS through the CSR of
//                        incoming edges, and d2 -- not a K = exp(..) buffer: the sweep reads d2 itself -- passes through LDS once in
//                        tiles of 64 x 64 doubles with a leading dimension of 65 and serves both directions: the column walk (lane = j,
//                        u -> v) reads 64 consecutive doubles and the row walk (lane = i, v -> u) has a stride of 65 doubles, both free
//                        of bank conflicts as documented there.  A tile is requested from memory one tile ahead, into 16 registers a
//                        thread: the first while h is built (three dependent reads deep), the next while this one is walked; a
//                        workgroup is latency, not bandwidth, and this changes no arithmetic.  A candidate is h[i] - g * d2[i, j], one multiply and one subtract
//                        formed per term from the tile (-ffp-contract=off), kept on strict > from -inf: a NaN never wins.  Where the
//                        sum of k_graph_sweep must keep its order and leaves two waves idle, all four waves work here: waves 0 and 1
//                        take the lower and the upper 32 source states of a tile for u -> v, waves 2 and 3 for v -> u, every one from
//                        -inf.  The two partial maxima of a tile are joined into the running maximum (LDS, av / au) in ascending order
//                        of the source state, lower half first, on strict >, by the threads that fetch the next tile: a later candidate
//                        replaces only if it is greater, exactly as the rule's single loop does, so even the sign of a zero maximum is
//                        the rule's.  top, the first maximum of u, is a reduction on (value, lowest index); nu' = u - top, the blend
//                        with damping, and the residual as in k_graph_sweep.  LDS per workgroup: the tile (33 280 B), four vectors of
//                        MAXN doubles, the partial maxima (2 048 B) and the reductions (160 B): 37 536 B for n <= 64 (MAXN = 64:
//                        4 workgroups, 16 waves, per CU of 160 KiB) and 43 680 B for n <= 256 (3 workgroups); 106 VGPRs allow 4 waves
//                        per SIMD as well (profiles/spatial_path/resource_usage.txt): LDS sets the occupancy, the registers fit it.
//   k_graph_maxmarginal  one workgroup per sounding, as k_graph_belief: theta_s plus all incoming messages, minus its first maximum; -inf
//                        for the states >= m_s.
//   k_graph_condition    one workgroup per (candidate, sounding of the launched level or colour), lane = state i: v[i] = theta_s[i]
//                        plus, per incoming edge in CSR order (ascending neighbour q), - g * d2 at the neighbour's state x_q if q is
//                        fixed, else the message nu[q -> s][i].  ALL_FIXED = false is the decode (fixed: level(q) < level(s); the
//                        state is set to the first maximum); ALL_FIXED = true is a step of the coordinate ascent (every neighbour is
//                        fixed; the state moves to the first maximum only if v there is strictly greater than v at the current state,
//                        and a move adds one to the launch's counter of the candidate: one integer atomic per workgroup, exact in any
//                        order).  s = ev[e] reads row x_q of the edge's slab, coalesced; s = eu[e] reads column x_q, strided by n: one
//                        64-byte sector per lane and edge, m_s of them.  That is paid, not staged: a column cannot be had with fewer
//                        sectors by going through LDS, and a workgroup reads each only once.  The first maximum is a reduction on
//                        (value, lowest index), ties to the lower state; a NaN or -inf never wins, and without a winner the state is 0.
//                        Soundings of one level that share an edge exchange messages, not states, and soundings of one colour share no
//                        edge: a launch reads no state that it writes.
// No grid barrier, no spin-wait, no float atomics: a call repeats its own bits.  Nothing outside the prefixes of d2 is read.  An index
// that does not fit (an endpoint or a listed sounding outside 0 .. S - 1, an entry of in_edge outside 0 .. 2 E - 1) is skipped, never
// followed; a neighbour's state is clamped into its prefix.
#pragma once

#include "gbp_section_graph.h"

namespace section {

constexpr int PATH_HALF = GRAPH_TILE / 2;

// theta_a[t] plus the messages into a, in_edge order (ascending neighbour), but the one of directed edge `skip`.
__device__ __forceinline__ double path_h(int a, int t, int n, long long twoE, long long skip, const double* __restrict__ score,
                                         const int* __restrict__ in_ptr, const int* __restrict__ in_edge, const double* __restrict__ nu)
{
    double h = score[(size_t)a * n + t];
    const int q1 = (int)min((long long)in_ptr[a + 1], twoE);
    for (int q = max(in_ptr[a], 0); q < q1; ++q) {
        const long long d = in_edge[q];
        if (d != skip && d >= 0 && d < twoE) h = h + nu[(size_t)d * n + t];
    }
    return h;
}

// (v, i) <- the better of (v, i) and (v2, i2): the greater value, the lower index among equals.  No value is a NaN here.
__device__ __forceinline__ void first_max_join(double& v, int& i, double v2, int i2)
{
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

// The first maximum of the workgroup's values on strict > from -inf: a NaN or -inf entry never wins (it enters as -inf), and without a
// winner the result is (-inf, 0) as thread 0's entry has the lowest index.  Every thread calls it with its own index; rv / ri hold
// WAVES entries and are free again after the next barrier.
__device__ __forceinline__ void block_first_max(double& v, int& i, double* rv, int* ri)
{
    if (!(v > -INFINITY)) v = -INFINITY;
    for (int off = 32; off > 0; off >>= 1) first_max_join(v, i, __shfl_xor(v, off), __shfl_xor(i, off));
    if ((threadIdx.x & 63) == 0) {
        rv[threadIdx.x >> 6] = v;
        ri[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = rv[0];
    i = ri[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) first_max_join(v, i, rv[w], ri[w]);
}

template <bool DAMP, int MAXN>
__global__ __launch_bounds__(THREADS) void k_graph_maxsum(int S, int E, int n, const int* __restrict__ eu, const int* __restrict__ ev,
                                                          const int* __restrict__ n_used, const double* __restrict__ score,
                                                          const double* __restrict__ g, const double* __restrict__ d2,
                                                          const int* __restrict__ in_ptr, const int* __restrict__ in_edge,
                                                          const double* __restrict__ nu_old, double* __restrict__ nu_new, double damping,
                                                          double* __restrict__ resid)
{
    __shared__ double tile[GRAPH_TILE * GRAPH_LD];
    __shared__ double hu[MAXN], hv[MAXN], au[MAXN], av[MAXN];               // n <= MAXN: 64 or 256
    __shared__ double part[2][2][GRAPH_TILE];                               // [direction][half of the tile's source states][lane]
    __shared__ double red[2 * WAVES], topv[2 * WAVES];
    __shared__ int topi[2 * WAVES];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t e = blockIdx.x;
    const long long twoE = 2 * (long long)E, d_uv = 2 * (long long)e, d_vu = d_uv + 1;
    const int u = eu[e], v = ev[e];
    if (u < 0 || u >= S || v < 0 || v >= S) {                               // (not an edge of this graph: its messages keep their values)
        if (t < 2) resid[d_uv + t] = 0.0;
        return;
    }
    const int mu = used(n_used, (size_t)u, n), mv = used(n_used, (size_t)v, n);
    const double* const D = d2 + e * (size_t)n * n;
    const int TI = (mu + GRAPH_TILE - 1) / GRAPH_TILE, TJ = (mv + GRAPH_TILE - 1) / GRAPH_TILE;
    double ahead[GRAPH_TILE / WAVES];                                       // this thread's entries of the tile to come, on their way
    auto request = [&](int tile_id) {                                       // (a tile past the last: nothing is read)
        const int ti = tile_id / TJ, tj = tile_id - ti * TJ;
        const int i0 = ti * GRAPH_TILE, ni = tile_id < TI * TJ ? min(GRAPH_TILE, mu - i0) : 0;
        const int j0 = tj * GRAPH_TILE, nj = min(GRAPH_TILE, mv - j0);
#pragma unroll
        for (int k = 0; k < GRAPH_TILE / WAVES; ++k) {
            const int ii = wave + WAVES * k;
            ahead[k] = (lane < nj && ii < ni) ? D[(size_t)(i0 + ii) * n + j0 + lane] : 0.0;
        }
    };
    request(0);                                                             // the first tile travels while h is built through the CSR
    if (t < mu) {
        hu[t] = path_h(u, t, n, twoE, d_vu, score, in_ptr, in_edge, nu_old);
        au[t] = -INFINITY;
    }
    if (t < mv) {
        hv[t] = path_h(v, t, n, twoE, d_uv, score, in_ptr, in_edge, nu_old);
        av[t] = -INFINITY;
    }
    const double ge = g[e];
    const int dir = wave >> 1, half = wave & 1;
    int pi0 = 0, pj0 = 0, pni = 0, pnj = 0;                                 // the tile before: its partial maxima wait in `part`
    for (int tile_id = 0; tile_id <= TI * TJ; ++tile_id) {                  // (one turn more: the last tile's partial maxima)
        const bool fetch = tile_id < TI * TJ;
        const int ti = tile_id / TJ, tj = tile_id - ti * TJ;
        const int i0 = ti * GRAPH_TILE, ni = fetch ? min(GRAPH_TILE, mu - i0) : 0;
        const int j0 = tj * GRAPH_TILE, nj = fetch ? min(GRAPH_TILE, mv - j0) : 0;
        __syncthreads();                                                    // h is whole; the last tile's readers are done, its partial maxima stand
        if (lane < nj) {
#pragma unroll
            for (int k = 0; k < GRAPH_TILE / WAVES; ++k) {
                const int ii = wave + WAVES * k;
                if (ii < ni) tile[ii * GRAPH_LD + lane] = ahead[k];
            }
        }
        if (fetch) request(tile_id + 1);                                    // the next tile travels while this one is walked
        if (wave == 0 && lane < pnj) {                                      // u -> v: column pj0 + lane, the source states ascending
            double a = av[pj0 + lane];
            const double lo = part[0][0][lane], hi = part[0][1][lane];
            if (lo > a) a = lo;
            if (hi > a) a = hi;
            av[pj0 + lane] = a;
        } else if (wave == 1 && lane < pni) {                               // v -> u: row pi0 + lane
            double a = au[pi0 + lane];
            const double lo = part[1][0][lane], hi = part[1][1][lane];
            if (lo > a) a = lo;
            if (hi > a) a = hi;
            au[pi0 + lane] = a;
        }
        __syncthreads();
        const int k0 = half * PATH_HALF;
        double p = -INFINITY;
        if (dir == 0) {                                                     // down column j0 + lane
            if (lane < nj) {
                const int k1 = min(ni, k0 + PATH_HALF);
#pragma unroll 8
                for (int ii = k0; ii < k1; ++ii) {
                    const double cand = hu[i0 + ii] - ge * tile[ii * GRAPH_LD + lane];
                    if (cand > p) p = cand;
                }
                part[0][half][lane] = p;
            }
        } else {                                                            // along row i0 + lane
            if (lane < ni) {
                const int k1 = min(nj, k0 + PATH_HALF);
#pragma unroll 8
                for (int jj = k0; jj < k1; ++jj) {
                    const double cand = hv[j0 + jj] - ge * tile[lane * GRAPH_LD + jj];
                    if (cand > p) p = cand;
                }
                part[1][half][lane] = p;
            }
        }
        pi0 = i0;
        pj0 = j0;
        pni = ni;
        pnj = nj;
    }
    __syncthreads();                                                        // (the turn past the last tile computed nothing: au and av are whole)
    double top_uv = t < mv ? av[t] : -INFINITY, top_vu = t < mu ? au[t] : -INFINITY;
    int at_uv = t, at_vu = t;
    block_first_max(top_uv, at_uv, topv, topi);
    block_first_max(top_vu, at_vu, topv + WAVES, topi + WAVES);
    double r_uv = 0.0, r_vu = 0.0;
    if (t < mv) {
        const double old = nu_old[(size_t)d_uv * n + t];
        double m = av[t] - top_uv;
        if (DAMP) m = (1.0 - damping) * m + damping * old;
        nu_new[(size_t)d_uv * n + t] = m;
        r_uv = fabs(m - old);
    }
    if (t < mu) {
        const double old = nu_old[(size_t)d_vu * n + t];
        double m = au[t] - top_vu;
        if (DAMP) m = (1.0 - damping) * m + damping * old;
        nu_new[(size_t)d_vu * n + t] = m;
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

__global__ __launch_bounds__(THREADS) void k_graph_maxmarginal(int E, int n, const int* __restrict__ n_used, const double* __restrict__ score,
                                                               const int* __restrict__ in_ptr, const int* __restrict__ in_edge,
                                                               const double* __restrict__ nu, double* __restrict__ max_marginal)
{
    __shared__ double topv[WAVES];
    __shared__ int topi[WAVES];
    const int t = (int)threadIdx.x;
    const size_t s = blockIdx.x;
    const int m = used(n_used, s, n);
    const double b = t < m ? path_h((int)s, t, n, 2 * (long long)E, -1, score, in_ptr, in_edge, nu) : -INFINITY;
    double top = b;
    int at = t;
    block_first_max(top, at, topv, topi);
    if (t < n) max_marginal[s * n + t] = t < m ? b - top : -INFINITY;
}

// Block b of a launch: candidate b / count, sounding node[b % count].  X [C, S]: the states; moves: the launch's counter of candidate 0,
// candidate c's lies moves_stride further on (ALL_FIXED only).  nu and level are read by the decode only.
template <bool ALL_FIXED>
__global__ __launch_bounds__(THREADS) void k_graph_condition(int S, int E, int n, const int* __restrict__ eu, const int* __restrict__ ev,
                                                             const int* __restrict__ n_used, const double* __restrict__ score,
                                                             const double* __restrict__ g, const double* __restrict__ d2,
                                                             const int* __restrict__ in_ptr, const int* __restrict__ in_edge,
                                                             const double* __restrict__ nu, const int* __restrict__ level,
                                                             const int* __restrict__ node, int count, int* __restrict__ X,
                                                             int* __restrict__ moves, int moves_stride)
{
    __shared__ double val[GRAPH_MAX_STATES];
    __shared__ double topv[WAVES];
    __shared__ int topi[WAVES];
    const int t = (int)threadIdx.x;
    const size_t cand = blockIdx.x / (unsigned)count;
    const int s = node[blockIdx.x % (unsigned)count];
    if (s < 0 || s >= S) return;
    int* const Xc = X + cand * (size_t)S;
    const int m = used(n_used, (size_t)s, n);
    const long long twoE = 2 * (long long)E;
    double v = -INFINITY;
    if (t < m) {
        v = score[(size_t)s * n + t];
        const int own = ALL_FIXED ? 0 : level[s];
        const int q1 = (int)min((long long)in_ptr[s + 1], twoE);
        for (int q = max(in_ptr[s], 0); q < q1; ++q) {
            const long long d = in_edge[q];
            if (d < 0 || d >= twoE) continue;
            const size_t e = (size_t)(d >> 1);
            const int nb = (d & 1) ? ev[e] : eu[e];                         // 2 e + 1 comes from ev[e] into eu[e] = s
            if (nb < 0 || nb >= S) continue;
            if (ALL_FIXED || level[nb] < own) {
                const int x = min(max(Xc[nb], 0), used(n_used, (size_t)nb, n) - 1);
                const double* const De = d2 + e * (size_t)n * n;
                v = v - g[e] * ((d & 1) ? De[(size_t)t * n + x] : De[(size_t)x * n + t]);
            } else {
                v = v + nu[(size_t)d * n + t];
            }
        }
    }
    if (ALL_FIXED) val[t] = v;
    double top = v;
    int at = t;
    block_first_max(top, at, topv, topi);                                   // (its barrier also makes val whole)
    if (t != 0) return;
    if (ALL_FIXED) {
        const int cur = min(max(Xc[s], 0), m - 1);
        if (top > val[cur]) {
            Xc[s] = at;
            atomicAdd(moves + cand * (size_t)moves_stride, 1);
        }
    } else {
        Xc[s] = at;
    }
}

}  // namespace section
