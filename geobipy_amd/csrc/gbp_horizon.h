// Horizon tracking along lines (geobipy_amd/horizons.py states the rule in numpy; include/geobipy_amd.h gbp_horizon_track): the most
// probable path and the smoothed marginals of a Markov chain over S depth cells (+ the state "absent", index S) per sequence.
//
// One 256-thread workgroup walks one sequence.  Thread t owns the states t + 256 j (NJ of them; the absent state is owned like a
// cell).  Per step the 2S - 1 transition costs T[k + S - 1], k = c' - c, are rebuilt in LDS; slot 2S - 1 holds the price of the
// switch.  An owner of cell c' reads T[c' + S - 1 - c] while c runs, a unit stride across lanes (no bank conflicts) beside the
// broadcast of V[c]; the owner of the absent state reads slot 2S - 1 with stride 0, so every lane runs the same loop.  V (or alpha)
// is double-buffered in LDS: two barriers per Viterbi step.  Every operation is one fp64 add, subtract, multiply or compare in the
// order of the rule (the library is built with -ffp-contract=off), so the path and its score equal numpy's in every bit.
#pragma once

namespace horizon {

constexpr int THREADS = 256;
constexpr int MAX_STATES = 2048;
constexpr int MAX_OWNED = (MAX_STATES + 1 + THREADS - 1) / THREADS;       // 9

// doubles of LDS a workgroup needs: two state vectors [S + 1], the table [2S] and four partial sums
inline size_t lds_doubles(int S) { return (size_t)4 * S + 2 + 4; }

// The sum of v over the workgroup, the same in every thread: lanes by butterfly, then the four waves in order.
__device__ inline double block_sum(double v, double* red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                                        // (the last sum's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// What a thread needs to know of the states it owns.  A slot past the last state reads the switch slot and stores nothing.
template <int NJ>
struct Owned {
    int cp[NJ], stride[NJ];
    bool live[NJ], cell[NJ];
    __device__ Owned(int S, int n_states)
    {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            cp[j] = (int)threadIdx.x + THREADS * j;
            live[j] = cp[j] < n_states;
            cell[j] = cp[j] < S;
            stride[j] = cell[j] ? 1 : 0;
        }
    }
};

template <int NJ>
__global__ __launch_bounds__(THREADS) void k_horizon_viterbi(const long long* __restrict__ ptr, int S, int has_absent, double dz,
                                                             const double* __restrict__ score, const double* __restrict__ absent_score,
                                                             const double* __restrict__ g, const double* __restrict__ d, double sw,
                                                             unsigned short* __restrict__ back, int* __restrict__ cell,
                                                             double* __restrict__ log_score)
{
    extern __shared__ double lds[];
    const int SA = S + 1, n_states = S + (has_absent ? 1 : 0), t = (int)threadIdx.x;
    double* Vc = lds;
    double* Vn = lds + SA;
    double* T = lds + 2 * SA;
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) {
        if (t == 0) log_score[blockIdx.x] = 0.0;
        return;
    }
    const Owned<NJ> own(S, n_states);
    // absent_score is read under the uniform has_absent only, never under a lane's condition: a uniform address is loaded by the
    // scalar unit, which does not look at the lanes' mask, and the pointer is NULL where there is no absent state
    double ab = has_absent ? absent_score[r0] : 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (own.live[j]) Vc[own.cp[j]] = own.cell[j] ? score[(size_t)r0 * S + own.cp[j]] : ab;
    if (t == 0) T[2 * S - 1] = sw;
    double gn = g[r0], dn = d[r0];
    for (int n = 0; n + 1 < N; ++n) {
        const size_t row = (size_t)r0 + n + 1;
        double sc[NJ];
        ab = has_absent ? absent_score[row] : 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) sc[j] = !own.live[j] ? 0.0 : own.cell[j] ? score[row * S + own.cp[j]] : ab;
        const double g_next = g[row], d_next = d[row];
        for (int k = t; k < 2 * S - 1; k += THREADS) T[k] = gn * fabs(dn - (double)(k - (S - 1)) * dz);
        __syncthreads();                                                    // T and V_n are whole
        double best[NJ];
        int arg[NJ], idx[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            best[j] = -INFINITY;
            arg[j] = 0;
            idx[j] = own.cell[j] ? own.cp[j] + S - 1 : 2 * S - 1;
        }
#pragma unroll 4
        for (int c = 0; c < S; ++c) {
            const double v = Vc[c];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const double cand = v - T[idx[j]];
                idx[j] -= own.stride[j];
                if (cand > best[j]) {                                       // strict: the first maximum stays
                    best[j] = cand;
                    arg[j] = c;
                }
            }
        }
        if (has_absent) {
            const double va = Vc[S];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const double cand = own.cell[j] ? va - sw : va;             // absent -> absent costs nothing
                if (cand > best[j]) {
                    best[j] = cand;
                    arg[j] = S;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (own.live[j]) {
                Vn[own.cp[j]] = sc[j] + best[j];
                back[row * (size_t)SA + own.cp[j]] = (unsigned short)arg[j];
            }
        __syncthreads();                                                    // V_{n+1} is whole; T and V_n are free
        double* tmp = Vc;
        Vc = Vn;
        Vn = tmp;
        gn = g_next;
        dn = d_next;
    }
    // the path back, by one lane: the pointers of a long line are tens of MB and stay on the device
    __threadfence();
    __syncthreads();
    if (t == 0) {
        __threadfence();
        int cur = 0;
        double top = Vc[0];
        for (int c = 1; c < n_states; ++c)
            if (Vc[c] > top) {
                top = Vc[c];
                cur = c;
            }
        log_score[blockIdx.x] = top;
        for (int n = N - 1; n >= 0; --n) {
            cell[r0 + n] = cur;
            if (n > 0) cur = (int)back[((size_t)r0 + n) * SA + cur];
        }
    }
}

// Scaled forward-backward.  Forward: alpha_n (normalised) goes to marginal row n and s_n to scale[n]; backward: beta_n is held in the
// owners' registers, u = w_{n+1} o beta_{n+1} in LDS, and gamma_n = alpha_n o beta_n, renormalised, replaces alpha_n in the row.
template <int NJ>
__global__ __launch_bounds__(THREADS) void k_horizon_marginals(const long long* __restrict__ ptr, int S, int has_absent, double dz,
                                                               const double* __restrict__ score, const double* __restrict__ absent_score,
                                                               const double* __restrict__ g, const double* __restrict__ d, double sw,
                                                               double* __restrict__ marginal, double* __restrict__ log_partition,
                                                               double* __restrict__ scale)
{
    extern __shared__ double lds[];
    const int SA = S + 1, n_states = S + (has_absent ? 1 : 0), t = (int)threadIdx.x;
    double* Ac = lds;
    double* An = lds + SA;
    double* K = lds + 2 * SA;
    double* red = K + 2 * S;
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) {
        if (t == 0) log_partition[blockIdx.x] = 0.0;
        return;
    }
    const Owned<NJ> own(S, n_states);
    const double ks = exp(-sw);
    if (t == 0) K[2 * S - 1] = ks;
    double u[NJ];
    // alpha_0 = w_0 / s_0 (absent_score: under the uniform has_absent only, as in the Viterbi kernel)
    double ab = has_absent ? absent_score[r0] : 0.0;
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        u[j] = !own.live[j] ? 0.0 : exp(own.cell[j] ? score[(size_t)r0 * S + own.cp[j]] : ab);
        part += u[j];
    }
    double s = block_sum(part, red);
    double lp = log(s);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (own.live[j]) {
            const double a = u[j] / s;
            Ac[own.cp[j]] = a;
            marginal[(size_t)r0 * n_states + own.cp[j]] = a;
        }
    if (t == 0) scale[r0] = s;
    double gn = g[r0], dn = d[r0];
    for (int n = 0; n + 1 < N; ++n) {
        const size_t row = (size_t)r0 + n + 1;
        double sc[NJ];
        ab = has_absent ? absent_score[row] : 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) sc[j] = !own.live[j] ? 0.0 : own.cell[j] ? score[row * S + own.cp[j]] : ab;
        const double g_next = g[row], d_next = d[row];
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
            u[j] = own.live[j] ? exp(sc[j]) * acc[j] : 0.0;
            part += u[j];
        }
        s = block_sum(part, red);                                           // (its barriers also free K and alpha_n)
        lp += log(s);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (own.live[j]) {
                const double a = u[j] / s;
                An[own.cp[j]] = a;
                marginal[row * n_states + own.cp[j]] = a;
            }
        if (t == 0) scale[row] = s;
        double* tmp = Ac;
        Ac = An;
        An = tmp;
        gn = g_next;
        dn = d_next;
    }
    if (t == 0) log_partition[blockIdx.x] = lp;
    // backward: every thread reads the scale its first lane wrote
    __threadfence();
    __syncthreads();
    __threadfence();
    double* U = Ac;                                                         // (alpha is read back from the rows: both vectors are free)
    double beta[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) beta[j] = 1.0;
    for (int n = N - 1; n >= 0; --n) {
        const size_t row = (size_t)r0 + n;
        if (n + 1 < N) {
            const double s_next = scale[row + 1];
            gn = g[row];
            dn = d[row];
            ab = has_absent ? absent_score[row + 1] : 0.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (own.live[j]) U[own.cp[j]] = exp(own.cell[j] ? score[(row + 1) * S + own.cp[j]] : ab) * beta[j];
            for (int k = t; k < 2 * S - 1; k += THREADS) K[k] = exp(-(gn * fabs(dn - (double)(k - (S - 1)) * dz)));
            __syncthreads();                                                // K and u are whole
            double acc[NJ];
            int idx[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                acc[j] = 0.0;
                idx[j] = own.cell[j] ? S - 1 - own.cp[j] : 2 * S - 1;       // K[c' - c + S - 1] with c' running
            }
#pragma unroll 4
            for (int c = 0; c < S; ++c) {
                const double v = U[c];
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    acc[j] = acc[j] + K[idx[j]] * v;
                    idx[j] += own.stride[j];
                }
            }
            if (has_absent) {
                const double ua = U[S];
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = acc[j] + (own.cell[j] ? ks * ua : ua);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) beta[j] = acc[j] / s_next;
        }
        double gm[NJ];
        part = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            gm[j] = own.live[j] ? marginal[row * n_states + own.cp[j]] * beta[j] : 0.0;
            part += gm[j];
        }
        const double tot = block_sum(part, red);                            // (its barriers also free K and u)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (own.live[j]) marginal[row * n_states + own.cp[j]] = gm[j] / tot;
    }
}

}  // namespace horizon
