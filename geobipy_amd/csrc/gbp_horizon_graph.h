// Horizons across flight lines (geobipy_amd/horizons.py propagate_reference and graph_path_reference state the rules in
// numpy; include/geobipy_amd.h gbp_horizon_graph_propagate, gbp_horizon_graph_path, gbp_horizon_graph_refine): synchronous message
// passing on the survey graph whose soundings all share S depth cells (+ the state "absent", index S; SA states in all).  The pair
// term of the undirected edge e = {u, v}, u < v, depends on the difference of the cell indices alone: cell a under u and cell b under
// v cost T_e[b - a] = g[e] * fabs(d[e] - (double)(b - a) * dz), cell <-> absent costs the switch, absent <-> absent nothing.  So an
// edge has a table of 2 S - 1 values where the section kernels (gbp_section_graph.h) stream an n x n matrix, and the states go up to
// 2 048 where theirs stop at 256.  Directed edge 2 e is u -> v, 2 e + 1 is v -> u; a message has SA entries.
//
//   k_hgraph_sweep   one launch per sweep, one 256-thread workgroup per UNDIRECTED edge, for both semirings: SUM (sum-product, linear
//                    domain, the table is K_e = exp(-T_e), the node term w = exp(score), a message is divided by its total) and max
//                    (max-sum, log domain, the table is T_e itself, the node term the score, a message has its first maximum taken
//                    off).  Dynamic LDS: hu [S + 1], hv [S + 1] and the table [2 S] (slot k + S - 1 for k = b - a; slot 2 S - 1 is
//                    the switch: ks = exp(-switch) or the switch): (4 S + 2) doubles, 65 552 B at S = 2 048, above the 48 KiB a launch
//                    gets without asking -- the opt-in of gbp_horizon_track.  The table is built once and serves both directions:
//                    for u -> v the owner of cell b reads slot b + S - 1 - a while a ascends, for v -> u the owner of cell a reads
//                    slot b - a + S - 1 while b ascends; either is a unit stride across the lanes (no bank conflict) beside the
//                    broadcast of h[source].  The owner of the absent state reads the switch slot with stride 0, so every lane runs
//                    the same loop.  hu and hv (the node term and all incoming messages but the partner's, the rule's order) are
//                    built through the CSR of incoming edges by section::graph_h / section::path_h.  A thread owns the states
//                    t + 256 j, j < NJ, as in k_horizon_viterbi, and holds both directions' results in registers; with SPLIT
//                    (SA <= 128, NJ = 1) threads 0 .. 127 take u -> v and threads 128 .. 255 take v -> u, state t & 127 each, so the
//                    two directions run side by side instead of one after the other on half-empty waves.  Once both are done the
//                    results replace hv (u -> v) and hu (v -> u) in LDS.  SUM: the total is summed by one lane per direction (lanes 0
//                    and 64: two waves), j ascending, the rule's loop.  Max: the first maximum is a reduction on (value, lowest
//                    index) -- the element the rule's loop from -inf on strict > ends on, whatever the order of the joins, so even
//                    the sign of a zero maximum is the rule's; a NaN or -inf never wins.  Every operation is one fp64 add,
//                    subtract, multiply, divide or compare of the rule (-ffp-contract=off); the max side has numpy's bits, the sum
//                    side differs by the device's exp alone.
//   k_hgraph_init    w = exp(score) [N, SA] and both message buffers = 1 / SA (SUM only; the max side starts from a memset of 0.0).
//   k_hgraph_node    one workgroup per sounding.  SUM: the belief, w times all incoming messages, divided by its total (one lane, i
//                    ascending), and its first maximum.  Max: the max-marginal, the score plus all incoming messages minus its first
//                    maximum.
//   k_hgraph_condition  the twin of section::k_graph_condition: one workgroup per (candidate, sounding of the launched level or
//                    colour), v[i] = score[s, i] and, per incoming edge in CSR order, minus the pair cost at the neighbour's state
//                    if that neighbour is decided, else plus its message; the first maximum of v; ALL_FIXED moves only to a strictly
//                    greater v and counts the move (one integer atomic per workgroup, exact in any order).
// No grid barrier, no float atomics: a call repeats its own bits.  An index that does not fit (an endpoint or a listed sounding
// outside 0 .. N - 1, an entry of in_edge outside 0 .. 2 E - 1) is skipped, never followed; a neighbour's state is clamped.
#pragma once

#include "gbp_horizon.h"
#include "gbp_section_graph_path.h"

namespace horizon_graph {

constexpr int THREADS = horizon::THREADS, WAVES = THREADS / 64, MAX_STATES = horizon::MAX_STATES, MAX_OWNED = horizon::MAX_OWNED;
constexpr int SPLIT_STATES = THREADS / 2;                                  // SA <= 128: a direction per half of the workgroup

static_assert(THREADS == section::THREADS, "section::block_first_max reduces a workgroup of section::THREADS");

inline size_t sweep_lds_bytes(int S) { return ((size_t)4 * S + 2) * sizeof(double); }

// One direction of an edge for the NJ states `own` holds: SUM: acc[j] = sum over the source cells c ascending of h[c] * K[slot], then
// h[S] * ks (a cell) or h[S] (the absent state); max: the maximum of h[c] - T[slot] on strict > from -inf, then h[S] - switch or h[S].
// MIRROR = false is u -> v (slot = own + S - 1 - c), true is v -> u (slot = c - own + S - 1).
template <bool SUM, bool MIRROR, int NJ>
__device__ __forceinline__ void edge_pass(const horizon::Owned<NJ>& own, int S, int has_absent, const double* __restrict__ h,
                                          const double* __restrict__ table, double (&acc)[NJ])
{
    int idx[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        acc[j] = SUM ? 0.0 : -INFINITY;
        idx[j] = !own.cell[j] ? 2 * S - 1 : MIRROR ? S - 1 - own.cp[j] : own.cp[j] + S - 1;
    }
#pragma unroll 4
    for (int c = 0; c < S; ++c) {
        const double v = h[c];
        double slot[NJ];                                                    // all NJ reads are issued before the first is waited for
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            slot[j] = table[idx[j]];
            idx[j] += MIRROR ? own.stride[j] : -own.stride[j];
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (SUM) {
                acc[j] = acc[j] + v * slot[j];
            } else {
                const double cand = v - slot[j];
                acc[j] = cand > acc[j] ? cand : acc[j];                     // strict: a NaN never wins
            }
        }
    }
    if (has_absent) {
        const double va = h[S], sw = table[2 * S - 1];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (SUM) {
                acc[j] = acc[j] + (own.cell[j] ? va * sw : va);             // absent -> absent costs nothing
            } else {
                const double cand = own.cell[j] ? va - sw : va;
                if (cand > acc[j]) acc[j] = cand;
            }
        }
    }
}

// The owned states of a thread that stands for lane `t` of a group (the whole workgroup, or a half of it with SPLIT).
template <int NJ>
__device__ __forceinline__ horizon::Owned<NJ> owned_by(int t, int S, int SA)
{
    horizon::Owned<NJ> own(S, SA);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        own.cp[j] = t + THREADS * j;
        own.live[j] = own.cp[j] < SA;
        own.cell[j] = own.cp[j] < S;
        own.stride[j] = own.cell[j] ? 1 : 0;
    }
    return own;
}

// node [N, SA]: w = exp(score) (SUM) or the score (max); old / new_ [2 E, SA]: the messages; resid [2 E] of this sweep.
template <bool SUM, bool DAMP, int NJ, bool SPLIT>
__global__ __launch_bounds__(THREADS) void k_hgraph_sweep(int N, int E, int S, int has_absent, double dz, double sw,
                                                          const int* __restrict__ eu, const int* __restrict__ ev,
                                                          const double* __restrict__ node, const double* __restrict__ g,
                                                          const double* __restrict__ d, const int* __restrict__ in_ptr,
                                                          const int* __restrict__ in_edge, const double* __restrict__ old,
                                                          double* __restrict__ new_, double damping, double* __restrict__ resid)
{
    static_assert(!SPLIT || NJ == 1, "a half of the workgroup owns one state per thread");
    extern __shared__ double lds[];
    __shared__ double red[2 * WAVES], topv[2 * WAVES], tot[2];
    __shared__ int topi[2 * WAVES];
    const int SA = S + (has_absent ? 1 : 0), t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    double* const hu = lds;
    double* const hv = lds + (S + 1);
    double* const table = lds + 2 * (S + 1);                                // [2 S]
    const size_t e = blockIdx.x;
    const long long twoE = 2 * (long long)E, d_uv = 2 * (long long)e, d_vu = d_uv + 1;
    const int u = eu[e], v = ev[e];
    if (u < 0 || u >= N || v < 0 || v >= N) {                               // (not an edge of this graph: its messages keep their values)
        if (t < 2) resid[d_uv + t] = 0.0;
        return;
    }
    const double ge = g[e], de = d[e];
    for (int k = t; k < 2 * S - 1; k += THREADS) {
        const double T = ge * fabs(de - (double)(k - (S - 1)) * dz);
        table[k] = SUM ? exp(-T) : T;
    }
    if (t == 0) table[2 * S - 1] = SUM ? exp(-sw) : sw;
    for (int c = t; c < SA; c += THREADS) {
        if (SUM) {
            hu[c] = section::graph_h(u, c, SA, twoE, d_vu, node, in_ptr, in_edge, old);
            hv[c] = section::graph_h(v, c, SA, twoE, d_uv, node, in_ptr, in_edge, old);
        } else {
            hu[c] = section::path_h(u, c, SA, twoE, d_vu, node, in_ptr, in_edge, old);
            hv[c] = section::path_h(v, c, SA, twoE, d_uv, node, in_ptr, in_edge, old);
        }
    }
    __syncthreads();                                                        // the table and both h are whole
    // with SPLIT a thread works for ONE direction (mine), else for both; a_uv belongs to the states of v, a_vu to those of u
    const int mine = SPLIT ? t / SPLIT_STATES : 0;
    const horizon::Owned<NJ> own = owned_by<NJ>(SPLIT ? t % SPLIT_STATES : t, S, SA);
    double a_uv[NJ], a_vu[NJ];
    if (!SPLIT || mine == 0) edge_pass<SUM, false, NJ>(own, S, has_absent, hu, table, a_uv);
    if (!SPLIT || mine == 1) edge_pass<SUM, true, NJ>(own, S, has_absent, hv, table, a_vu);
    __syncthreads();                                                        // both h are free
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (own.live[j]) {
            if (!SPLIT || mine == 0) hv[own.cp[j]] = a_uv[j];
            if (!SPLIT || mine == 1) hu[own.cp[j]] = a_vu[j];
        }
    double top_uv = -INFINITY, top_vu = -INFINITY;
    if (SUM) {
        __syncthreads();
        if (t == 0) {                                                       // the rule's order: one lane, ascending
            double s = 0.0;
            for (int j = 0; j < SA; ++j) s = s + hv[j];
            tot[0] = s;
        } else if (t == 64) {
            double s = 0.0;
            for (int i = 0; i < SA; ++i) s = s + hu[i];
            tot[1] = s;
        }
        __syncthreads();
    } else {
        int at_uv = 0x7fffffff, at_vu = 0x7fffffff;                         // (a thread without a state of a direction never wins its ties)
#pragma unroll
        for (int j = 0; j < NJ; ++j)                                        // ascending index: strict > keeps the first
            if (own.live[j]) {
                if ((!SPLIT || mine == 0) && a_uv[j] > top_uv) {
                    top_uv = a_uv[j];
                    at_uv = own.cp[j];
                }
                if ((!SPLIT || mine == 1) && a_vu[j] > top_vu) {
                    top_vu = a_vu[j];
                    at_vu = own.cp[j];
                }
            }
        section::block_first_max(top_uv, at_uv, topv, topi);
        section::block_first_max(top_vu, at_vu, topv + WAVES, topi + WAVES);
    }
    double r_uv = 0.0, r_vu = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (own.live[j]) {
            const size_t c = (size_t)own.cp[j];
            if (!SPLIT || mine == 0) {
                const double was = old[(size_t)d_uv * SA + c];
                double m = SUM ? a_uv[j] / tot[0] : a_uv[j] - top_uv;
                if (DAMP) m = (1.0 - damping) * m + damping * was;
                new_[(size_t)d_uv * SA + c] = m;
                r_uv = section::nan_max(r_uv, fabs(m - was));
            }
            if (!SPLIT || mine == 1) {
                const double was = old[(size_t)d_vu * SA + c];
                double m = SUM ? a_vu[j] / tot[1] : a_vu[j] - top_vu;
                if (DAMP) m = (1.0 - damping) * m + damping * was;
                new_[(size_t)d_vu * SA + c] = m;
                r_vu = section::nan_max(r_vu, fabs(m - was));
            }
        }
    r_uv = section::wave_nan_max(r_uv);
    r_vu = section::wave_nan_max(r_vu);
    if (lane == 0) {
        red[wave] = r_uv;
        red[WAVES + wave] = r_vu;
    }
    __syncthreads();
    if (t < 2)
        resid[d_uv + t] = section::nan_max(section::nan_max(section::nan_max(red[WAVES * t], red[WAVES * t + 1]), red[WAVES * t + 2]),
                                           red[WAVES * t + 3]);
}

// w [N, SA] = exp(score); both message buffers [2 E, SA] = 1 / SA.  Block b < N is a sounding, block N + d a directed edge.
__global__ __launch_bounds__(THREADS) void k_hgraph_init(int N, int SA, const double* __restrict__ score, double* __restrict__ w,
                                                         double* __restrict__ mu0, double* __restrict__ mu1)
{
    const int t = (int)threadIdx.x;
    if ((int)blockIdx.x < N) {
        const size_t s = blockIdx.x;
        for (int c = t; c < SA; c += THREADS) w[s * SA + c] = exp(score[s * SA + c]);
        return;
    }
    const size_t dir = (size_t)blockIdx.x - (size_t)N;
    const double first = 1.0 / (double)SA;
    for (int c = t; c < SA; c += THREADS) {
        mu0[dir * SA + c] = first;
        mu1[dir * SA + c] = first;
    }
}

// SUM: out = the belief and state its first maximum; max: out = the max-marginal (state is not written).
template <bool SUM>
__global__ __launch_bounds__(THREADS) void k_hgraph_node(int E, int SA, const double* __restrict__ node, const int* __restrict__ in_ptr,
                                                         const int* __restrict__ in_edge, const double* __restrict__ msg,
                                                         double* __restrict__ out, int* __restrict__ state)
{
    __shared__ double h[MAX_STATES + 1];
    __shared__ double tot, topv[WAVES];
    __shared__ int topi[WAVES];
    const int t = (int)threadIdx.x;
    const size_t s = blockIdx.x;
    const long long twoE = 2 * (long long)E;
    double top = -INFINITY;
    int at = 0x7fffffff;
    for (int c = t; c < SA; c += THREADS) {                                 // ascending index: strict > keeps the first
        const double b = SUM ? section::graph_h((int)s, c, SA, twoE, -1, node, in_ptr, in_edge, msg)
                             : section::path_h((int)s, c, SA, twoE, -1, node, in_ptr, in_edge, msg);
        h[c] = b;
        if (!SUM && b > top) {
            top = b;
            at = c;
        }
    }
    if (!SUM) {
        section::block_first_max(top, at, topv, topi);                      // (its barrier comes after every h is written by its own thread)
        for (int c = t; c < SA; c += THREADS) out[s * SA + c] = h[c] - top;
        return;
    }
    __syncthreads();
    if (t == 0) {
        double a = 0.0;
        for (int i = 0; i < SA; ++i) a = a + h[i];
        tot = a;
    }
    __syncthreads();
    for (int c = t; c < SA; c += THREADS) {
        h[c] = h[c] / tot;
        out[s * SA + c] = h[c];
    }
    __syncthreads();
    if (t == 0) {                                                           // the first maximum: strict >, a NaN never replaces
        int cur = 0;
        double best = h[0];
        for (int i = 1; i < SA; ++i)
            if (h[i] > best) {
                best = h[i];
                cur = i;
            }
        state[s] = cur;
    }
}

// The cost between state i of sounding s and state x of its neighbour over edge e; `mirror`: s = eu[e] (i is cell a, x is cell b).
__device__ __forceinline__ double pair_cost(int i, int x, bool mirror, int S, double ge, double de, double dz, double sw)
{
    if (i < S && x < S) return ge * fabs(de - (double)(mirror ? x - i : i - x) * dz);
    return (i >= S && x >= S) ? 0.0 : sw;
}

// Block b of a launch: candidate b / count, sounding list[b % count].  X [C, N]: the states; moves: the launch's counter of candidate 0,
// candidate c's lies moves_stride further on (ALL_FIXED only).  msg and level are read by the decode only.
template <bool ALL_FIXED>
__global__ __launch_bounds__(THREADS) void k_hgraph_condition(int N, int E, int S, int has_absent, double dz, double sw,
                                                              const int* __restrict__ eu, const int* __restrict__ ev,
                                                              const double* __restrict__ score, const double* __restrict__ g,
                                                              const double* __restrict__ d, const int* __restrict__ in_ptr,
                                                              const int* __restrict__ in_edge, const double* __restrict__ msg,
                                                              const int* __restrict__ level, const int* __restrict__ list, int count,
                                                              int* __restrict__ X, int* __restrict__ moves, int moves_stride)
{
    __shared__ double topv[WAVES], at_current;
    __shared__ int topi[WAVES];
    const int SA = S + (has_absent ? 1 : 0), t = (int)threadIdx.x;
    const size_t cand = blockIdx.x / (unsigned)count;
    const int s = list[blockIdx.x % (unsigned)count];
    if (s < 0 || s >= N) return;
    int* const Xc = X + cand * (size_t)N;
    const long long twoE = 2 * (long long)E;
    const int own_level = ALL_FIXED ? 0 : level[s];
    const int cur = ALL_FIXED ? min(max(Xc[s], 0), SA - 1) : 0;
    const int q0 = max(in_ptr[s], 0), q1 = (int)min((long long)in_ptr[s + 1], twoE);
    double top = -INFINITY;
    int at = 0x7fffffff;
    for (int i = t; i < SA; i += THREADS) {                                 // ascending index: strict > keeps the first
        double v = score[(size_t)s * SA + i];
        for (int q = q0; q < q1; ++q) {
            const long long dir = in_edge[q];
            if (dir < 0 || dir >= twoE) continue;
            const size_t e = (size_t)(dir >> 1);
            const int nb = (dir & 1) ? ev[e] : eu[e];                       // 2 e + 1 comes from ev[e] into eu[e] = s
            if (nb < 0 || nb >= N) continue;
            if (ALL_FIXED || level[nb] < own_level) {
                const int x = min(max(Xc[nb], 0), SA - 1);
                v = v - pair_cost(i, x, (dir & 1) != 0, S, g[e], d[e], dz, sw);
            } else {
                v = v + msg[(size_t)dir * SA + i];
            }
        }
        if (ALL_FIXED && i == cur) at_current = v;
        if (v > top) {
            top = v;
            at = i;
        }
    }
    section::block_first_max(top, at, topv, topi);                          // (its barrier also makes at_current visible)
    if (t != 0) return;
    if (at < 0 || at >= SA) at = 0;                                         // (no winner)
    if (ALL_FIXED) {
        if (top > at_current) {
            Xc[s] = at;
            atomicAdd(moves + cand * (size_t)moves_stride, 1);
        }
    } else {
        Xc[s] = at;
    }
}

}  // namespace horizon_graph
