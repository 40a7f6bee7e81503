// Joint draws across flight lines (geobipy_amd/sections.py graph_draw_reference states the rule in numpy;
// include/geobipy_amd.h gbp_section_graph_draw): Gibbs sampling on the survey graph of gbp_section_graph.h, blocked by flight line.
// A block is one sequence of ptr.  Given the states of the neighbouring lines a line is a chain whose conditional is drawn exactly by
// the forward filter and the backward sampling of gbp_section.h: every cross-line edge of a sounding s multiplies its weights by one
// column (s = ev) or one row (s = eu) of K_e, taken at the neighbour's current state.  Lines that share no cross edge form a colour
// class and are drawn by one pair of launches.  Realisations are independent chains, realisation = lane.
//
//   k_graph_weights      w = exp(score) [S, n] on the prefix, 0.0 beyond.
//   k_graph_line_filter  one 256-thread workgroup per (sequence of the colour, realisation); n <= 256, so thread j owns state j.  It is
//                        forward_rows' loop with two differences: the step matrix is read from the K that k_graph_kernel wrote,
//                        through step_edge (no exp per term), and thread j builds w'[j] from w and the CSR of the sounding's incoming
//                        cross edges: one read of K per cross edge, coalesced where s = ev, strided by n where s = eu.  alpha goes to
//                        filtered [R, S, n] and the normaliser to scale [R, S].  LDS: (2 n + 4) doubles, dynamic.
//   k_graph_line_draw    one wave per (sequence of the colour, 64 realisations), lane = realisation: k_section_draw's walk with alpha
//                        indexed by the realisation and K read in place of exp(-(g d2)); the cumulative sum is formed twice in the
//                        rule's order, as there.  The states live in draw_state [R, S] itself and are replaced in place.
// A launch of colour c reads only states of other colours and writes only its own: no atomics, no order that depends on scheduling;
// a call repeats its own bits.  u = u53(x, y) of philox(seed, rho, key low, key high, sweep): a draw depends on the seed, the
// realisation, the sounding's key and the sweep, not on how many realisations a call holds or how they are cut into blocks.
// An index that does not fit (an edge outside 0 .. E - 1, a sounding outside 0 .. S - 1, a sequence outside 0 .. L - 1) is skipped,
// never followed; a neighbour's state is clamped into its prefix.  Every operation is one multiply, add, divide or compare as the
// rule writes it (-ffp-contract=off).
#pragma once

#include "gbp_section_graph.h"

namespace section {

__global__ __launch_bounds__(THREADS) void k_graph_weights(int n, const int* __restrict__ n_used, const double* __restrict__ score,
                                                           double* __restrict__ w)
{
    const int t = (int)threadIdx.x;
    const size_t s = blockIdx.x;
    const int m = used(n_used, s, n);
    if (t < n) w[s * n + t] = t < m ? exp(score[s * n + t]) : 0.0;
}

// The sequence block b of a launch works on: b itself at the start sweep (lines == NULL), else the b-th sequence of the colour; -1: none.
__device__ __forceinline__ int graph_line_of(int b, int L, const int* __restrict__ colour_ptr, const int* __restrict__ colour_line, int colour)
{
    if (!colour_line) return b;
    const int c0 = colour_ptr[colour], c1 = colour_ptr[colour + 1];
    if (c0 < 0 || c1 > L || b >= c1 - c0) return -1;
    const int line = colour_line[c0 + b];
    return line >= 0 && line < L ? line : -1;
}

// w'_s[j]: w_s[j] times, for every incoming cross edge of s in CSR order (ascending neighbour), K_e[j, x_q] (s = eu[e]) or
// K_e[x_q, j] (s = ev[e]), x_q the neighbour's state in this realisation (X).  j < m_s.
template <bool COND>
__device__ __forceinline__ double graph_cond_weight(size_t s, int j, int S, int E, int n, const int* __restrict__ eu, const int* __restrict__ ev,
                                                    const int* __restrict__ n_used, const double* __restrict__ w, const double* __restrict__ K,
                                                    const int* __restrict__ cross_ptr, const int* __restrict__ cross_edge,
                                                    const int* __restrict__ X)
{
    double v = w[s * n + j];
    if (COND) {
        const long long twoE = 2 * (long long)E;
        const int q1 = (int)min((long long)cross_ptr[s + 1], twoE);
        for (int q = max(cross_ptr[s], 0); q < q1; ++q) {
            const long long d = cross_edge[q];
            if (d < 0 || d >= twoE) continue;
            const size_t e = (size_t)(d >> 1);
            const int nb = (d & 1) ? ev[e] : eu[e];                         // 2 e + 1 comes from ev[e] into eu[e] = s
            if (nb < 0 || nb >= S) continue;
            const int x = min(max(X[nb], 0), used(n_used, (size_t)nb, n) - 1);
            const double* const Ke = K + e * (size_t)n * n;
            v = v * ((d & 1) ? Ke[(size_t)j * n + x] : Ke[(size_t)x * n + j]);
        }
    }
    return v;
}

template <bool COND>
__global__ __launch_bounds__(THREADS) void k_graph_line_filter(int S, int E, int n, int L, const long long* __restrict__ ptr,
                                                               const int* __restrict__ eu, const int* __restrict__ ev,
                                                               const int* __restrict__ n_used, const double* __restrict__ w,
                                                               const double* __restrict__ K, const int* __restrict__ step_edge,
                                                               const int* __restrict__ cross_ptr, const int* __restrict__ cross_edge,
                                                               const int* __restrict__ colour_ptr, const int* __restrict__ colour_line,
                                                               int colour, const int* __restrict__ draw_state,
                                                               double* __restrict__ filtered, double* __restrict__ scale)
{
    extern __shared__ double lds[];
    const int t = (int)threadIdx.x;
    const int line = graph_line_of((int)(blockIdx.x % (unsigned)L), L, colour_ptr, colour_line, colour);
    if (line < 0) return;
    const size_t rb = blockIdx.x / (unsigned)L;                             // the realisation within the call
    const long long r0 = ptr[line];
    const int N = (int)(ptr[line + 1] - r0);
    if (N <= 0 || r0 < 0 || r0 + N > S) return;
    const int* const X = draw_state + rb * (size_t)S;
    double* const rows = filtered + rb * (size_t)S * n;
    double* const sc = scale + rb * (size_t)S;
    double* Ac = lds;
    double* An = lds + n;
    double* red = lds + 2 * n;
    int m = used(n_used, (size_t)r0, n);
    double u = t < m ? graph_cond_weight<COND>((size_t)r0, t, S, E, n, eu, ev, n_used, w, K, cross_ptr, cross_edge, X) : 0.0;
    double s = horizon::block_sum(u, red);
    if (t < n) {
        const double a = t < m ? u / s : 0.0;
        Ac[t] = a;
        rows[(size_t)r0 * n + t] = a;
    }
    if (t == 0) sc[r0] = s;
    for (int st = 0; st + 1 < N; ++st) {
        const size_t r = (size_t)r0 + st;
        const int mn = used(n_used, r + 1, n);
        const int se = step_edge[r];
        const bool step = se >= 0 && se < E;                                // (no such edge: the sum stays 0.0, nothing is read)
        const double* const Ke = K + (step ? (size_t)se : 0) * (size_t)n * n;
        const double wn = t < mn ? graph_cond_weight<COND>(r + 1, t, S, E, n, eu, ev, n_used, w, K, cross_ptr, cross_edge, X) : 0.0;
        __syncthreads();                                                    // alpha_r is whole
        double acc = 0.0;
        const int jc = min(t, mn - 1);
        if (step) {
#pragma unroll 8
            for (int i = 0; i < m; ++i) acc = acc + Ac[i] * Ke[(size_t)i * n + jc];      // (eight rows of K on their way: a step is latency)
        }
        u = t < mn ? wn * acc : 0.0;
        s = horizon::block_sum(u, red);                                     // (its barriers also free alpha_r's readers)
        if (t < n) {
            const double a = t < mn ? u / s : 0.0;
            An[t] = a;
            rows[(r + 1) * n + t] = a;
        }
        if (t == 0) sc[r + 1] = s;
        double* tmp = Ac;
        Ac = An;
        An = tmp;
        m = mn;
    }
}

// Backward sampling of the sequences of a colour (sections.graph_draw_reference states the rule): k_section_draw's walk, lane =
// realisation.  first_draw + the lane's index in the call is rho, the realisation's number in the Philox counter; a lane past n_draws
// walks along the last realisation's alpha and stores nothing.  No LDS, no barrier.
__global__ __launch_bounds__(64) void k_graph_line_draw(int S, int E, int n, int L, const long long* __restrict__ ptr,
                                                        const int* __restrict__ n_used, const double* __restrict__ K,
                                                        const int* __restrict__ step_edge, const int* __restrict__ colour_ptr,
                                                        const int* __restrict__ colour_line, int colour,
                                                        const long long* __restrict__ row_key, unsigned long long seed, int n_draws,
                                                        int first_draw, unsigned sweep, const double* __restrict__ filtered,
                                                        int* __restrict__ draw_state)
{
    const int line = graph_line_of((int)(blockIdx.x % (unsigned)L), L, colour_ptr, colour_line, colour);
    if (line < 0) return;
    const long long r0 = ptr[line];
    const int N = (int)(ptr[line + 1] - r0);
    if (N <= 0 || r0 < 0 || r0 + N > S) return;
    const unsigned local = (blockIdx.x / (unsigned)L) * 64u + threadIdx.x;
    const bool live = local < (unsigned)n_draws;
    const size_t rb = live ? local : (unsigned)n_draws - 1u;
    const unsigned rho = (unsigned)first_draw + local;
    const double* const rows = filtered + rb * (size_t)S * n;
    int* const X = draw_state + rb * (size_t)S;
    int j = 0;
    for (int st = N - 1; st >= 0; --st) {
        const size_t r = (size_t)r0 + st;
        const int m = used(n_used, r, n);
        const unsigned long long key = row_key ? (unsigned long long)row_key[r] : (unsigned long long)r;
        const rng::U4 x = rng::philox(seed, rho, (uint32_t)key, (uint32_t)(key >> 32), sweep);
        const double u = rng::u53(x.x, x.y);
        const double* const A = rows + r * (size_t)n;
        const int se = st == N - 1 ? -1 : step_edge[r];
        const bool last = se < 0 || se >= E;                                // the sequence's last sounding (or no such edge: alpha alone)
        const double* const Kc = K + (last ? 0 : (size_t)se) * (size_t)n * n + j;      // column j of K; not read at the last sounding
        double c = 0.0;
        if (last)
            for (int i = 0; i < m; ++i) c = c + A[i];
        else
#pragma unroll 4
            for (int i = 0; i < m; ++i) c = c + A[i] * Kc[(size_t)i * n];
        const double thr = u * c;
        int pick = 0;
        c = 0.0;
        if (last)
            for (int i = 0; i < m; ++i) {
                c = c + A[i];
                pick += c <= thr ? 1 : 0;
            }
        else
#pragma unroll 4
            for (int i = 0; i < m; ++i) {
                c = c + A[i] * Kc[(size_t)i * n];
                pick += c <= thr ? 1 : 0;
            }
        j = min(pick, m - 1);
        if (live) X[r] = j;
    }
}

}  // namespace section
