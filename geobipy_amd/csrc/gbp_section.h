// Sections of sampled models along a line (geobipy_amd/sections.py track_reference states the rule in numpy;
// include/geobipy_amd.h gbp_section_track): the most probable path and the smoothed marginals of a Markov chain whose states are the
// kept models of each sounding -- m_r = n_used[r] of n -- and whose transition r -> r + 1 is the dense matrix g[r] * d2[r, i, j].
//
// One 256-thread workgroup walks one sequence; V (or alpha) is double-buffered in LDS.
//   k_section_viterbi<NJ>    thread t owns the states (t mod W) + 256 jj.  Per step it walks i upward over column j of d2[r]: a wave
//                            reads 64 consecutive doubles of row i beside the broadcast of V[i].  With n <= 128 only n lanes would own
//                            a state, so the G = 256 / W lane groups (W = 64, 128 or 256 >= n) each take a contiguous part of the i
//                            range and meet in LDS in ascending order, strict > to replace: the first maximum, as in one loop.  Every
//                            operation is one fp64 multiply, subtract, add or compare as the rule writes it (-ffp-contract=off): the
//                            path and its score equal numpy's in every bit.  The walk back is one lane's.
//   k_section_marginals<NJ>  scaled forward-backward.  Forward as above (columns, i ascending, no lane groups).  The backward pass needs
//                            rows of d2[r]: a wave per state i, its lanes over 64 consecutive j, a butterfly to add them up.
//   k_section_filter<NJ>     the forward half alone (forward_rows, the device function both kernels run), for the draws.
//   k_section_draw           joint draws of whole sections by backward sampling: one wave per (sequence, 64 realisations), lane =
//                            realisation; see the kernel.
// Nothing outside the prefixes i < m_r, j < m_{r+1} is read.  No atomics.
#pragma once

#include "gbp_horizon.h"
#include "gbp_philox.h"

namespace section {

constexpr int THREADS = 256, MAX_STATES = 1024, MAX_OWNED = MAX_STATES / THREADS, WAVES = THREADS / 64, MAX_DRAWS = 65536;

inline size_t lds_bytes(int n) { return (size_t)(2 * n + WAVES) * sizeof(double); }        // two state vectors and four partial sums

__device__ __forceinline__ int used(const int* n_used, size_t r, int n) { return min(max(n_used[r], 1), n); }

template <int NJ>
__global__ __launch_bounds__(THREADS) void k_section_viterbi(const long long* __restrict__ ptr, int n, int W, const int* __restrict__ n_used,
                                                             const double* __restrict__ score, const double* __restrict__ g,
                                                             const double* __restrict__ d2, unsigned short* __restrict__ back,
                                                             int* __restrict__ state, double* __restrict__ log_score)
{
    constexpr int IN_FLIGHT = NJ == 1 ? 16 : 8;                             // rows of d2 a lane has on their way: a step is latency, not bandwidth
    extern __shared__ double lds[];
    __shared__ double part_best[THREADS];
    __shared__ int part_arg[THREADS];
    const int t = (int)threadIdx.x, G = THREADS / W, col = t & (W - 1), part = t / W;
    double* Vc = lds;
    double* Vn = lds + n;
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) {
        if (t == 0) log_score[blockIdx.x] = 0.0;
        return;
    }
    int m = used(n_used, (size_t)r0, n);
    if (part == 0) {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = col + THREADS * jj;
            if (j < m) Vc[j] = score[(size_t)r0 * n + j];
        }
    }
    __syncthreads();
    int mn = N > 1 ? used(n_used, (size_t)r0 + 1, n) : 1;
    double gr = g[r0];
    for (int s = 0; s + 1 < N; ++s) {
        const size_t r = (size_t)r0 + s;
        const int m_after = s + 2 < N ? used(n_used, r + 2, n) : 1;         // the next step's, asked for a step ahead: nobody waits for them
        const double g_next = g[r + 1];
        const int chunk = (m + G - 1) / G, i0 = part * chunk, i1 = min(m, i0 + chunk);
        const double* const D = d2 + r * (size_t)n * n;
        double best[NJ], sc[NJ];
        int arg[NJ], jc[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            best[jj] = -INFINITY;
            arg[jj] = 0;
            jc[jj] = min(col + THREADS * jj, mn - 1);                       // (a lane without a state walks the last column: no read outside the prefix)
            sc[jj] = score[(r + 1) * n + jc[jj]];
        }
#pragma clang loop unroll_count(IN_FLIGHT)
        for (int i = i0; i < i1; ++i) {                                     // (the loads of d2 do not wait for the compares: IN_FLIGHT rows at once)
            const double v = Vc[i];
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const double cand = v - gr * D[(size_t)i * n + jc[jj]];
                if (cand > best[jj]) {                                      // strict: the first maximum stays, a NaN never wins
                    best[jj] = cand;
                    arg[jj] = i;
                }
            }
        }
        if (G > 1) {                                                        // (NJ == 1: the lane groups meet, the lower part of i first)
            part_best[t] = best[0];
            part_arg[t] = arg[0];
            __syncthreads();
            if (part == 0)
                for (int p = 1; p < G; ++p) {
                    const double ob = part_best[p * W + col];
                    if (ob > best[0]) {
                        best[0] = ob;
                        arg[0] = part_arg[p * W + col];
                    }
                }
        }
        if (part == 0) {
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int j = col + THREADS * jj;
                if (j < mn) {
                    Vn[j] = sc[jj] + best[jj];
                    back[(r + 1) * n + j] = (unsigned short)arg[jj];
                }
            }
        }
        __syncthreads();                                                    // V_{r+1} is whole; V_r and the parts are free
        double* tmp = Vc;
        Vc = Vn;
        Vn = tmp;
        m = mn;
        mn = m_after;
        gr = g_next;
    }
    // the path back, by one lane: the pointers stay on the device
    __threadfence();
    __syncthreads();
    if (t == 0) {
        __threadfence();
        int cur = 0;
        double top = Vc[0];
        for (int j = 1; j < m; ++j)
            if (Vc[j] > top) {
                top = Vc[j];
                cur = j;
            }
        log_score[blockIdx.x] = top;
        for (int s = N - 1; s >= 0; --s) {
            state[r0 + s] = cur;
            if (s > 0) cur = min((int)back[((size_t)r0 + s) * n + cur], n - 1);
        }
    }
}

// The forward half of the scaled forward-backward pass, shared by k_section_marginals and k_section_filter (one copy of the arithmetic:
// the same bits through either kernel): alpha_r (normalised; 0.0 for the states >= m_r) goes to row r of `rows` [T, n] and s_r to
// scale[r]; returns sum ln s_r.  Every thread of the 256-thread workgroup calls it; lds holds (2 n + WAVES) doubles, all free afterwards
// once the workgroup has met at a barrier.
template <int NJ>
__device__ __forceinline__ double forward_rows(double* lds, long long r0, int N, int n, const int* __restrict__ n_used,
                                               const double* __restrict__ score, const double* __restrict__ g,
                                               const double* __restrict__ d2, double* __restrict__ rows, double* __restrict__ scale)
{
    const int t = (int)threadIdx.x;
    double* Ac = lds;
    double* An = lds + n;
    double* red = lds + 2 * n;
    int m = used(n_used, (size_t)r0, n);
    double u[NJ];
    double part = 0.0;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = t + THREADS * jj;
        u[jj] = j < m ? exp(score[(size_t)r0 * n + j]) : 0.0;
        part += u[jj];
    }
    double s = horizon::block_sum(part, red);
    double lp = log(s);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = t + THREADS * jj;
        if (j < n) {
            const double a = j < m ? u[jj] / s : 0.0;
            Ac[j] = a;
            rows[(size_t)r0 * n + j] = a;
        }
    }
    if (t == 0) scale[r0] = s;
    for (int st = 0; st + 1 < N; ++st) {
        const size_t r = (size_t)r0 + st;
        const int mn = used(n_used, r + 1, n);
        const double gr = g[r];
        const double* const D = d2 + r * (size_t)n * n;
        __syncthreads();                                                    // alpha_r is whole
        double acc[NJ];
        int jc[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            acc[jj] = 0.0;
            jc[jj] = min(t + THREADS * jj, mn - 1);
        }
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const double a = Ac[i];
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) acc[jj] = acc[jj] + a * exp(-(gr * D[(size_t)i * n + jc[jj]]));
        }
        part = 0.0;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = t + THREADS * jj;
            u[jj] = j < mn ? exp(score[(r + 1) * n + j]) * acc[jj] : 0.0;
            part += u[jj];
        }
        s = horizon::block_sum(part, red);                                  // (its barriers also free alpha_r's readers)
        lp += log(s);
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = t + THREADS * jj;
            if (j < n) {
                const double a = j < mn ? u[jj] / s : 0.0;
                An[j] = a;
                rows[(r + 1) * n + j] = a;
            }
        }
        if (t == 0) scale[r + 1] = s;
        double* tmp = Ac;
        Ac = An;
        An = tmp;
        m = mn;
    }
    return lp;
}

// Scaled forward-backward.  Forward: forward_rows into the marginal rows; backward: beta_r lives in LDS, u = w_{r+1} o beta_{r+1}
// beside it, and gamma_r = alpha_r o beta_r, renormalised, replaces alpha_r in the row.
template <int NJ>
__global__ __launch_bounds__(THREADS) void k_section_marginals(const long long* __restrict__ ptr, int n, const int* __restrict__ n_used,
                                                               const double* __restrict__ score, const double* __restrict__ g,
                                                               const double* __restrict__ d2, double* __restrict__ marginal,
                                                               double* __restrict__ log_partition, double* __restrict__ scale)
{
    extern __shared__ double lds[];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    double* red = lds + 2 * n;
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) {
        if (t == 0) log_partition[blockIdx.x] = 0.0;
        return;
    }
    const double lp = forward_rows<NJ>(lds, r0, N, n, n_used, score, g, d2, marginal, scale);
    int m = used(n_used, (size_t)r0 + N - 1, n);
    double part;
    if (t == 0) log_partition[blockIdx.x] = lp;
    // backward: every thread reads the scale its first lane wrote
    __threadfence();
    __syncthreads();
    __threadfence();
    double* Bt = lds;                                                       // (alpha is read back from the rows: both vectors are free)
    double* U = lds + n;
    for (int j = t; j < n; j += THREADS) Bt[j] = 1.0;
    __syncthreads();
    int mn = m;                                                             // m_{r+1} while r runs down; m is m_{N-1} here
    for (int st = N - 1; st >= 0; --st) {
        const size_t r = (size_t)r0 + st;
        m = used(n_used, r, n);
        if (st + 1 < N) {
            const double s_next = scale[r + 1], gr = g[r];
            const double* const D = d2 + r * (size_t)n * n;
            for (int j = t; j < mn; j += THREADS) U[j] = exp(score[(r + 1) * n + j]) * Bt[j];
            __syncthreads();                                                // u is whole; beta_{r+1} is free
            for (int i = wave; i < m; i += WAVES) {
                double acc = 0.0;
                for (int j = lane; j < mn; j += 64) acc = acc + exp(-(gr * D[(size_t)i * n + j])) * U[j];
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
                if (lane == 0) Bt[i] = acc / s_next;
            }
            __syncthreads();                                                // beta_r is whole
        }
        double gm[NJ];
        part = 0.0;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = t + THREADS * jj;
            gm[jj] = j < m ? marginal[r * n + j] * Bt[j] : 0.0;
            part += gm[jj];
        }
        const double tot = horizon::block_sum(part, red);                   // (its barriers also free u)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = t + THREADS * jj;
            if (j < m) marginal[r * n + j] = gm[jj] / tot;
        }
        mn = m;
    }
}

// The filter alone: the rows of alpha_r (what a backward SAMPLING pass needs, where the smoothed marginals need beta) and the steps'
// normalisers.  forward_rows is the whole kernel.
template <int NJ>
__global__ __launch_bounds__(THREADS) void k_section_filter(const long long* __restrict__ ptr, int n, const int* __restrict__ n_used,
                                                            const double* __restrict__ score, const double* __restrict__ g,
                                                            const double* __restrict__ d2, double* __restrict__ filtered,
                                                            double* __restrict__ scale)
{
    extern __shared__ double lds[];
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) return;
    forward_rows<NJ>(lds, r0, N, n, n_used, score, g, d2, filtered, scale);
}

// Backward sampling (sections.draw_reference states the rule).  One wave per (sequence, 64 realisations), lane = realisation rho; the
// walk runs r = last .. first of the sequence.  Per step a lane holds j, its state under r + 1, and runs i upward over column j of
// d2[r]: alpha_r[i] is the same address in every lane and the 64 reads of d2[r, i, j_lane] fall within row i.  The cumulative sum is
// formed twice in the rule's order, c = c + alpha_r[i] * exp(-(g[r] * d2[r, i, j])) with i ascending: once for its total (the
// threshold is u * total), once more to count the i with c <= threshold -- the same operations on the same operands, so the same c.
// The count is capped at m_r - 1; with a NaN total no comparison holds and the pick is 0.  u = u53(x, y) of philox(seed, rho, key low,
// key high, 0), key = row_key[r] (NULL: r): a draw depends on the seed, the realisation and the row's key, not on the launch.  A lane
// past n_draws walks along and stores nothing.  No atomics, no LDS, no barrier; draw_state is int32 [n_draws, total_n].
__global__ __launch_bounds__(64) void k_section_draw(const long long* __restrict__ ptr, long long total_n, int n, const int* __restrict__ n_used,
                                                     const double* __restrict__ g, const double* __restrict__ d2,
                                                     const long long* __restrict__ row_key, unsigned long long seed, int n_draws,
                                                     const double* __restrict__ filtered, int* __restrict__ draw_state)
{
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) return;
    const unsigned rho = blockIdx.y * 64u + threadIdx.x;
    const bool live = rho < (unsigned)n_draws;
    int j = 0;
    for (int st = N - 1; st >= 0; --st) {
        const size_t r = (size_t)r0 + st;
        const int m = used(n_used, r, n);
        const unsigned long long key = row_key ? (unsigned long long)row_key[r] : (unsigned long long)r;
        const rng::U4 x = rng::philox(seed, rho, (uint32_t)key, (uint32_t)(key >> 32), 0u);
        const double u = rng::u53(x.x, x.y);
        const double* const A = filtered + r * (size_t)n;
        const bool last = st == N - 1;
        const double gr = last ? 0.0 : g[r];
        const double* const D = d2 + r * (size_t)n * n + j;                 // column j of d2[r]; not read at the sequence's last row
        double c = 0.0;
        if (last)
            for (int i = 0; i < m; ++i) c = c + A[i];
        else
#pragma unroll 4
            for (int i = 0; i < m; ++i) c = c + A[i] * exp(-(gr * D[(size_t)i * n]));
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
                c = c + A[i] * exp(-(gr * D[(size_t)i * n]));
                pick += c <= thr ? 1 : 0;
            }
        j = min(pick, m - 1);
        if (live) draw_state[(size_t)rho * (size_t)total_n + r] = j;
    }
}

}  // namespace section
