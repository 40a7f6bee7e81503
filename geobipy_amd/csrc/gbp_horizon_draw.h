// Joint draws of horizons (geobipy_amd/horizons.py draw_reference and graph_draw_reference state the rules in numpy;
// include/geobipy_amd.h gbp_horizon_draw, gbp_horizon_graph_draw): forward filtering and backward sampling of the chain
// of gbp_horizon.h -- S depth cells (+ the state "absent", index S), a pair term that is a table of 2S - 1 values per step, no matrix
// -- along lines, and Gibbs sampling blocked by flight line on the survey graph, where the cross edges of a sounding multiply its
// weights by the pair factor at the neighbours' current states.
//
//   k_horizon_filter<NJ, COND>  one 256-thread workgroup per sequence (COND false), or per (sequence of the colour, realisation) (COND
//                         true): the forward loop of horizon::k_horizon_marginals written again (that kernel is left as it is), thread
//                         t owns the states t + 256 j, K_n rebuilt in LDS per step with ks in slot 2S - 1, alpha double-buffered in
//                         LDS.  With COND the owner of state i builds w' from the cross CSR: one exp per (state, cross edge); there is
//                         no [E, S, S] buffer.  alpha_n goes to the rows of the realisation, s_n to scale.
//   k_horizon_walk<SHARED>  lane = realisation, up to 256 realisations per workgroup, one workgroup per (sequence, group of
//                         realisations).  Per step the workgroup rebuilds K_n in LDS (2S doubles); with SHARED (the line draw and the
//                         start sweep) it stages the one alpha row beside it (S + 1 doubles) and every lane loops i over LDS alone,
//                         without it the lanes read their own alpha rows from the workspace.  K is read at slot j_lane - i + S - 1,
//                         and a lane whose j is absent reads the switch slot with stride 0, so every lane runs one loop.  The
//                         cumulative sum is formed twice in the rule's order, once for its total and once to count c <= thr: the
//                         same operations on the same operands, so the same c.
//
// Every operation is one fp64 multiply, add, divide, fabs, exp or compare as the rule writes it (the library is built with
// -ffp-contract=off).  No atomics, no grid barrier: a launch of a colour reads only states of other colours and writes its own, and a
// call repeats its bits.  absent_score, row_key, step_edge and colour_line may be NULL and are read under launch-uniform conditions
// only (the scalar unit that loads a uniform address does not look at the lanes' mask).  An index that does not fit (an edge, a
// sounding, a sequence, a colour) is skipped, never followed; a neighbour's state is clamped into 0 .. n_states - 1.
#pragma once

namespace horizon_draw {

constexpr int THREADS = horizon::THREADS;
constexpr int MAX_DRAWS = 65536;
constexpr int MAX_SWEEPS = 65535;

// doubles of LDS: the filter needs what the marginals need; the walk the table [2S] and, shared, one state vector [S + 1]
inline size_t filter_lds_doubles(int S) { return horizon::lds_doubles(S); }
inline size_t walk_lds_doubles(int S, bool shared) { return (size_t)2 * S + (shared ? S + 1 : 0); }

// The sequence block b works on: b itself where there are no colour lists (lines == NULL), else the b-th sequence of the colour; -1: none.
__device__ __forceinline__ int line_of(int b, int L, const int* __restrict__ colour_ptr, const int* __restrict__ colour_line, int colour)
{
    if (!colour_line) return b < L ? b : -1;
    const int c0 = colour_ptr[colour], c1 = colour_ptr[colour + 1];
    if (c0 < 0 || c1 > L || b >= c1 - c0) return -1;
    const int line = colour_line[c0 + b];
    return line >= 0 && line < L ? line : -1;
}

// g and d of the step row -> row + 1: the row's own entry along a line (step_edge == NULL), the step edge's on the graph; a row
// without a step edge (a sequence's last) gives 1 and 0, which nothing reads.
__device__ __forceinline__ void step_terms(size_t row, int E, const double* __restrict__ g, const double* __restrict__ d,
                                           const int* __restrict__ step_edge, double& gn, double& dn)
{
    if (!step_edge) {
        gn = g[row];
        dn = d[row];
        return;
    }
    const int se = step_edge[row];
    const bool ok = se >= 0 && se < E;
    gn = ok ? g[se] : 1.0;
    dn = ok ? d[se] : 0.0;
}

// w'_s: wv[j] (= w_s of the owned states) times, for every incoming cross edge of s in CSR order (ascending neighbour), the pair factor
// at the neighbour's state x: exp(-(g_e |d_e - k dz|)) between cells, k = x - i where s = eu[e] (the id 2 e + 1 comes from ev[e]) and
// i - x where s = ev[e]; ks between a cell and absent; no multiply between absent and absent.
template <int NJ>
__device__ __forceinline__ void cond_weights(double (&wv)[NJ], const horizon::Owned<NJ>& own, size_t s, int N, int E, int S, int n_states, double dz,
                                             double ks, const int* __restrict__ eu, const int* __restrict__ ev, const double* __restrict__ g,
                                             const double* __restrict__ d, const int* __restrict__ cross_ptr, const int* __restrict__ cross_edge,
                                             const int* __restrict__ X)
{
    const long long twoE = 2 * (long long)E;
    const int q1 = (int)min((long long)cross_ptr[s + 1], twoE);
    for (int q = max(cross_ptr[s], 0); q < q1; ++q) {
        const long long dd = cross_edge[q];
        if (dd < 0 || dd >= twoE) continue;
        const size_t e = (size_t)(dd >> 1);
        const bool from_v = (dd & 1) != 0;                                  // the neighbour is ev[e], s = eu[e]
        const int nb = from_v ? ev[e] : eu[e];
        if (nb < 0 || nb >= N) continue;
        const int x = min(max(X[nb], 0), n_states - 1);
        const double ge = g[e], de = d[e];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (!own.live[j]) continue;
            if (own.cell[j]) {
                if (x < S) {
                    const int k = from_v ? x - own.cp[j] : own.cp[j] - x;
                    wv[j] = wv[j] * exp(-(ge * fabs(de - (double)k * dz)));
                } else
                    wv[j] = wv[j] * ks;
            } else if (x < S)
                wv[j] = wv[j] * ks;
        }
    }
}

// score is [n_total, S] with absent_score [n_total] beside it (the line entry), or [n_total, n_states] with the absent state's column
// last (absent_score == NULL: the graph entry).
template <int NJ, bool COND>
__global__ __launch_bounds__(THREADS) void k_horizon_filter(const long long* __restrict__ ptr, int L, long long n_total, int E, int S, int has_absent,
                                                            double dz, const double* __restrict__ score, const double* __restrict__ absent_score,
                                                            const double* __restrict__ g, const double* __restrict__ d, double sw,
                                                            const int* __restrict__ step_edge, const int* __restrict__ eu,
                                                            const int* __restrict__ ev, const int* __restrict__ cross_ptr,
                                                            const int* __restrict__ cross_edge, const int* __restrict__ colour_ptr,
                                                            const int* __restrict__ colour_line, int colour, const int* __restrict__ draw_state,
                                                            double* __restrict__ filtered, double* __restrict__ scale)
{
    extern __shared__ double lds[];
    const int SA = S + 1, n_states = S + (has_absent ? 1 : 0), t = (int)threadIdx.x;
    double* Ac = lds;
    double* An = lds + SA;
    double* K = lds + 2 * SA;
    double* red = K + 2 * S;
    const int line = line_of((int)(blockIdx.x % (unsigned)L), L, colour_ptr, colour_line, colour);
    if (line < 0) return;
    const size_t rb = blockIdx.x / (unsigned)L;                             // the realisation within the call (0 without COND)
    const long long r0 = ptr[line];
    const int N = (int)(ptr[line + 1] - r0);
    if (N <= 0 || r0 < 0 || r0 + N > n_total) return;                       // (an empty sequence: nothing is written)
    const int* const X = COND ? draw_state + rb * (size_t)n_total : nullptr;
    double* const rows = filtered + rb * (size_t)n_total * n_states;
    double* const sc_out = scale + rb * (size_t)n_total;
    const size_t stride = absent_score ? (size_t)S : (size_t)n_states;
    const horizon::Owned<NJ> own(S, n_states);
    const double ks = exp(-sw);
    if (t == 0) K[2 * S - 1] = ks;
    double u[NJ];
    // the absent state's score: under the uniform has_absent and the uniform absent_score only, never under a lane's condition
    double ab = !has_absent ? 0.0 : absent_score ? absent_score[r0] : score[(size_t)r0 * stride + S];
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) u[j] = !own.live[j] ? 0.0 : exp(own.cell[j] ? score[(size_t)r0 * stride + own.cp[j]] : ab);
    if (COND) cond_weights<NJ>(u, own, (size_t)r0, (int)n_total, E, S, n_states, dz, ks, eu, ev, g, d, cross_ptr, cross_edge, X);
#pragma unroll
    for (int j = 0; j < NJ; ++j) part += u[j];
    double s = horizon::block_sum(part, red);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (own.live[j]) {
            const double a = u[j] / s;
            Ac[own.cp[j]] = a;
            rows[(size_t)r0 * n_states + own.cp[j]] = a;
        }
    if (t == 0) sc_out[r0] = s;
    double gn, dn;
    step_terms((size_t)r0, E, g, d, step_edge, gn, dn);
    for (int n = 0; n + 1 < N; ++n) {
        const size_t row = (size_t)r0 + n + 1;
        double wn[NJ];
        ab = !has_absent ? 0.0 : absent_score ? absent_score[row] : score[row * stride + S];
#pragma unroll
        for (int j = 0; j < NJ; ++j) wn[j] = !own.live[j] ? 0.0 : exp(own.cell[j] ? score[row * stride + own.cp[j]] : ab);
        if (COND) cond_weights<NJ>(wn, own, row, (int)n_total, E, S, n_states, dz, ks, eu, ev, g, d, cross_ptr, cross_edge, X);
        double g_next, d_next;
        step_terms(row, E, g, d, step_edge, g_next, d_next);
        for (int k = t; k < 2 * S - 1; k += THREADS) K[k] = exp(-(gn * fabs(dn - (double)(k - (S - 1)) * dz)));
        __syncthreads();                                                    // K and alpha_n are whole
        double acc[NJ];
        int idx[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            acc[j] = 0.0;
            idx[j] = own.cell[j] ? own.cp[j] + S - 1 : 2 * S - 1;
        }
#pragma unroll 4
        for (int c = 0; c < S; ++c) {
            const double a = Ac[c];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                acc[j] = acc[j] + a * K[idx[j]];
                idx[j] -= own.stride[j];
            }
        }
        if (has_absent) {
            const double aa = Ac[S];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = acc[j] + (own.cell[j] ? aa * ks : aa);
        }
        part = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            u[j] = own.live[j] ? wn[j] * acc[j] : 0.0;
            part += u[j];
        }
        s = horizon::block_sum(part, red);                                  // (its barriers also free K and alpha_n)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (own.live[j]) {
                const double a = u[j] / s;
                An[own.cp[j]] = a;
                rows[row * n_states + own.cp[j]] = a;
            }
        if (t == 0) sc_out[row] = s;
        double* tmp = Ac;
        Ac = An;
        An = tmp;
        gn = g_next;
        dn = d_next;
    }
}

// Backward sampling (horizons.draw_reference and graph_draw_reference state the rule).  The lane's realisation within the call is
// local = blockIdx.y * 256 + threadIdx.x and rho = first_draw + local its number in the Philox counter; it walks n = N - 1 .. 0 of the
// sequence of blockIdx.x; j is its state under n + 1.  u = u53(x, y) of philox(seed, rho, key low, key high, sweep), key = row_key[n]
// (NULL: n).  A lane past n_draws walks along (the last realisation's rows without SHARED) and stores nothing.  draw_state is int32
// [n_draws, n_total], S meaning absent; without SHARED filtered is [n_draws, n_total, n_states], with it [n_total, n_states].
template <bool SHARED>
__global__ __launch_bounds__(THREADS) void k_horizon_walk(const long long* __restrict__ ptr, int L, long long n_total, int E, int S, int has_absent,
                                                          double dz, const double* __restrict__ g, const double* __restrict__ d, double sw,
                                                          const int* __restrict__ step_edge, const int* __restrict__ colour_ptr,
                                                          const int* __restrict__ colour_line, int colour,
                                                          const long long* __restrict__ row_key, unsigned long long seed, int n_draws,
                                                          int first_draw, unsigned sweep, const double* __restrict__ filtered,
                                                          int* __restrict__ draw_state)
{
    extern __shared__ double lds[];
    const int n_states = S + (has_absent ? 1 : 0), t = (int)threadIdx.x;
    double* K = lds;                                                        // [2S]: the table, the switch in slot 2S - 1
    double* As = lds + 2 * S;                                               // [S + 1]: alpha_n, with SHARED only
    const int line = line_of((int)blockIdx.x, L, colour_ptr, colour_line, colour);
    if (line < 0) return;
    const long long r0 = ptr[line];
    const int N = (int)(ptr[line + 1] - r0);
    if (N <= 0 || r0 < 0 || r0 + N > n_total) return;
    const unsigned local = blockIdx.y * (unsigned)THREADS + threadIdx.x;
    const bool live = local < (unsigned)n_draws;
    const size_t rb = live ? local : (unsigned)n_draws - 1u;
    const unsigned rho = (unsigned)first_draw + local;
    const double ks = exp(-sw);
    if (t == 0) K[2 * S - 1] = ks;
    int j = 0;
    for (int st = N - 1; st >= 0; --st) {
        const size_t r = (size_t)r0 + st;
        const bool last = st == N - 1;
        if (!last) {
            double gn, dn;
            step_terms(r, E, g, d, step_edge, gn, dn);
            for (int k = t; k < 2 * S - 1; k += THREADS) K[k] = exp(-(gn * fabs(dn - (double)(k - (S - 1)) * dz)));
        }
        if (SHARED)
            for (int i = t; i < n_states; i += THREADS) As[i] = filtered[r * (size_t)n_states + i];
        __syncthreads();                                                    // K (and alpha_n) are whole
        const double* const A = SHARED ? (const double*)As : filtered + (rb * (size_t)n_total + r) * (size_t)n_states;
        const unsigned long long key = row_key ? (unsigned long long)row_key[r] : (unsigned long long)r;
        const rng::U4 x = rng::philox(seed, rho, (uint32_t)key, (uint32_t)(key >> 32), sweep);
        const double u = rng::u53(x.x, x.y);
        const bool jc = j < S;                                              // the state under n + 1 is a cell
        const int stride = jc ? 1 : 0, top = jc ? j + S - 1 : 2 * S - 1;
        const double aa = has_absent ? A[S] : 0.0;                          // (slot S exists only with the absent state)
        const double wa = (last || !jc) ? aa : aa * ks;                     // absent -> absent: no multiply
        double c = 0.0;
        int idx = top;
        if (last)
            for (int i = 0; i < S; ++i) c = c + A[i];
        else
#pragma unroll 4
            for (int i = 0; i < S; ++i) {
                c = c + A[i] * K[idx];
                idx -= stride;
            }
        if (has_absent) c = c + wa;
        const double thr = u * c;
        int pick = 0;
        c = 0.0;
        idx = top;
        if (last)
            for (int i = 0; i < S; ++i) {
                c = c + A[i];
                pick += c <= thr ? 1 : 0;
            }
        else
#pragma unroll 4
            for (int i = 0; i < S; ++i) {
                c = c + A[i] * K[idx];
                idx -= stride;
                pick += c <= thr ? 1 : 0;
            }
        if (has_absent) {
            c = c + wa;
            pick += c <= thr ? 1 : 0;
        }
        j = min(pick, n_states - 1);
        if (live) draw_state[rb * (size_t)n_total + r] = j;
        __syncthreads();                                                    // every lane is done with K and alpha_n
    }
}

}  // namespace horizon_draw
