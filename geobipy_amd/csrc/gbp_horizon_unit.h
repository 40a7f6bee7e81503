// Horizon pairs: the top and the base of one unit tracked jointly and ordered (geobipy_amd/horizons.py unit_reference states the rule in
// numpy; include/geobipy_amd.h gbp_horizon_unit_track).  The state under a sounding is a pair (a, b) of cells of one
// window of S cells, valid when b - a >= min_cells, or "absent"; a step costs T[a' - a] + T[b' - b], which is separable, so the
// transition over S^2 states is two passes of S^3 operations instead of one of S^4:
//   pass 1 (rows):    M1[a'][b]  = max / sum over a ascending of V[a][b]   (-, *) T[a' - a]
//   pass 2 (columns): M2[a'][b'] = max / sum over b ascending of M1[a'][b] (-, *) T[b' - b]
//
// One 512-thread workgroup walks one sequence; the S x S matrix V (alpha, or u = w o beta) and the matrix of pass 1 are two buffers in
// dynamic LDS beside the 2 S table of the step, the node scores of the next sounding and the scratch of the reductions:
// (2 S^2 + 5 S + 16 + 1024) doubles, 159 616 B at S = 96 of the 163 840 B of a CU (S = 98 does not fit) -- hence MAX_UNIT_STATES = 96.  Invalid pairs hold
// -inf (weight 0 in the linear domain) where a pass can read them, and whole rows and columns of them are skipped by loop bounds that
// are uniform in a wave: a -inf candidate never wins a strict >, and adding an exact 0 changes no bit.
//
// Lanes.  In both passes the lanes of a wave run along the base index (the column c of the matrix, lane = c mod 64) and a wave works
// on JA = 4 rows at a time, which are uniform in the wave.  Pass 1 reads V[a][c] at unit stride across the lanes -- 8-byte reads are
// served in two groups of 32 lanes, and 32 consecutive doubles cover the 64 banks once: no conflict -- and T[a' - a] at one address
// (a broadcast) per row.  Pass 2 reads M1[a'][b] at one address per row and T[c - b] at unit stride.  The stores go to [row][c],
// unit stride again.  The flat passes (the normalisation, the absent state's reductions, gamma) run over i = t + 512 j, unit stride.
// The thickness projection reads B[a][a + k] with the lanes along k: (S + 1) a + k, unit stride.  No access of the kernel has a stride
// other than 0 or 1 across a wave.
//
// Arithmetic.  Every Viterbi operation is one fp64 add, subtract, multiply or compare in the order of the rule (the library is built
// with -ffp-contract=off), so the paths and their score equal numpy's in every bit; the first maximum over the pairs in row-major
// order is found by a reduction whose ties go to the smaller flat index, which is the same pair.  The sums of the two passes add in
// the rule's order; the normalising sums, the absent state's sums over the pairs and the three projections of gamma are reduced by
// lanes and waves, in another order than numpy's.  No atomics, no spin-waits: a call repeats its bits.
//
// Workspaces (the caller's): back uint8 [2, total_n, S, S] -- the argument of pass 1 at [row][a'][b], then that of pass 2 at
// [row][a'][b'] (S: the pair was entered from the absent state) --, back_absent int32 [total_n] (the flat index of the pair the absent
// state was entered from; S^2: it stayed absent), and for the marginals alpha f64 [total_n, S^2 + 1], the absent state last.
#pragma once

namespace horizon_unit {

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_UNIT_STATES = 96;
constexpr int JA = 4;                                                       // rows a thread works on at a time

// doubles of LDS a workgroup needs: two matrices, the table [2S], score_top, score_base and thickness_score [S] each, the partial
// results of the waves (a double and an int each) and the partial projections of every thread (base and thickness)
inline size_t lds_doubles(int S) { return (size_t)2 * S * S + 5 * (size_t)S + 2 * WAVES + 2 * THREADS; }

// Where a thread sits: column c (lanes along the base index), row group r of R; the columns of a wave end at wave_cmax.
struct Geom {
    int S, mc, c, cc, r, R, wave_cmax;
    bool live;
    __device__ Geom(int S_, int mc_) : S(S_), mc(mc_)
    {
        const int BW = S <= 64 ? 64 : 128, t = (int)threadIdx.x;
        c = t % BW;
        r = t / BW;
        R = THREADS / BW;
        live = c < S;
        cc = live ? c : S - 1;                                              // (a lane past the last column reads the last and stores nothing)
        wave_cmax = min(S - 1, c | 63);
    }
};

__device__ inline double block_sum(double v, double* red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                                        // (the last reduction's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = s + red[w];
    return s;
}

// The first maximum in the order of the index i, the same in every thread: a larger value wins, an equal one with a smaller index.
__device__ inline void first_max(double& v, int& i, double ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

__device__ inline void block_first_max(double& v, int& i, double* redv, int* redi)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        first_max(v, i, ov, oi);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        redv[threadIdx.x >> 6] = v;
        redi[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = redv[0];
    i = redi[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) first_max(v, i, redv[w], redi[w]);
}

// Pass 1: out[x][c] = max (SUM: sum) over i = 0 .. wave_cmax - mc ascending of In[i][c] - (SUM: *) Tab[S - 1 + sgn (x - i)] for the rows
// x = 0 .. S - 1 - mc (a later row has no valid pair); done(x, c, value, argument) stores one result.
template <bool SUM, class Done>
__device__ inline void pass_rows(const double* In, const double* Tab, const Geom& q, int sgn, Done done)
{
    const int S = q.S, row_max = S - 1 - q.mc, i_hi = q.wave_cmax - q.mc;
    for (int x0 = q.r; x0 <= row_max; x0 += q.R * JA) {
        int x[JA], tb[JA], arg[JA];
        double acc[JA];
#pragma unroll
        for (int j = 0; j < JA; ++j) {
            x[j] = min(x0 + q.R * j, row_max);                              // (a row past the last repeats it and is not stored)
            tb[j] = S - 1 + sgn * x[j];
            acc[j] = SUM ? 0.0 : -INFINITY;
            arg[j] = 0;
        }
        for (int i = 0; i <= i_hi; ++i) {
            const double v = In[i * S + q.cc];
#pragma unroll
            for (int j = 0; j < JA; ++j) {
                const double tv = Tab[tb[j]];
                tb[j] -= sgn;
                if (SUM) {
                    acc[j] = acc[j] + v * tv;
                } else {
                    const double cand = v - tv;
                    if (cand > acc[j]) {                                    // strict: the first maximum stays
                        acc[j] = cand;
                        arg[j] = i;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < JA; ++j)
            if (q.live && x0 + q.R * j <= row_max) done(x[j], q.c, acc[j], arg[j]);
    }
}

// Pass 2: out[x][c] = max (SUM: sum) over i = mc .. S - 1 ascending of In[x][i] - (SUM: *) Tab[S - 1 + sgn (c - i)] for the rows
// x = 0 .. wave_cmax - mc (under a later row the wave's columns hold no valid pair, and no pass reads them).
template <bool SUM, class Done>
__device__ inline void pass_cols(const double* In, const double* Tab, const Geom& q, int sgn, Done done)
{
    const int S = q.S, row_max = q.wave_cmax - q.mc;
    for (int x0 = q.r; x0 <= row_max; x0 += q.R * JA) {
        int x[JA], arg[JA];
        double acc[JA];
#pragma unroll
        for (int j = 0; j < JA; ++j) {
            x[j] = min(x0 + q.R * j, row_max);
            acc[j] = SUM ? 0.0 : -INFINITY;
            arg[j] = 0;
        }
        int tb = S - 1 + sgn * (q.cc - q.mc);
        for (int i = q.mc; i < S; ++i) {
            const double tv = Tab[tb];
            tb -= sgn;
#pragma unroll
            for (int j = 0; j < JA; ++j) {
                const double m = In[x[j] * S + i];
                if (SUM) {
                    acc[j] = acc[j] + m * tv;
                } else {
                    const double cand = m - tv;
                    if (cand > acc[j]) {
                        acc[j] = cand;
                        arg[j] = i;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < JA; ++j)
            if (q.live && x0 + q.R * j <= row_max) done(x[j], q.c, acc[j], arg[j]);
    }
}

// The carve of the dynamic LDS.
struct Lds {
    double *A, *B, *Tab, *ST, *SB, *TS, *redv, *part;
    int* redi;
    __device__ Lds(double* lds, int S)
    {
        A = lds;
        B = A + S * S;
        Tab = B + S * S;
        ST = Tab + 2 * S;
        SB = ST + S;
        TS = SB + S;
        redv = TS + S;
        redi = (int*)(redv + WAVES);
        part = redv + 2 * WAVES;
    }
};

// The node score of the pair (a, b) from the rows in LDS: (top + base) + thickness, the last term only where it is given.
__device__ inline double node_score(const Lds& m, int has_ts, int a, int b)
{
    const double s = m.ST[a] + m.SB[b];
    return has_ts ? s + m.TS[b - a] : s;
}

__device__ inline void load_rows(const Lds& m, int S, const double* score_top, const double* score_base, size_t row)
{
    for (int k = (int)threadIdx.x; k < S; k += THREADS) {
        m.ST[k] = score_top[row * S + k];
        m.SB[k] = score_base[row * S + k];
    }
}

__global__ __launch_bounds__(THREADS) void k_unit_viterbi(const long long* __restrict__ ptr, int S, int mc, int has_absent, int has_ts, double dz,
                                                          const double* __restrict__ score_top, const double* __restrict__ score_base,
                                                          const double* __restrict__ thickness_score, const double* __restrict__ absent_score,
                                                          const double* __restrict__ g, const double* __restrict__ d, double sw,
                                                          unsigned char* __restrict__ back1, unsigned char* __restrict__ back2,
                                                          int* __restrict__ back_absent, int* __restrict__ cell_top, int* __restrict__ cell_base,
                                                          double* __restrict__ log_score)
{
    extern __shared__ double lds[];
    const int t = (int)threadIdx.x, SS = S * S;
    const Lds m(lds, S);
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) {
        if (t == 0) log_score[blockIdx.x] = 0.0;
        return;
    }
    const Geom q(S, mc);
    load_rows(m, S, score_top, score_base, (size_t)r0);
    if (has_ts)
        for (int k = t; k < S; k += THREADS) m.TS[k] = thickness_score[k];
    __syncthreads();
    for (int i = t; i < SS; i += THREADS) {
        const int a = i / S, b = i - a * S;
        m.A[i] = b - a >= mc ? node_score(m, has_ts, a, b) : -INFINITY;
    }
    // absent_score is read under the uniform has_absent only (the pointer is NULL where there is no absent state)
    double Va = has_absent ? absent_score[r0] : -INFINITY;
    double gn = g[r0], dn = d[r0];
    __syncthreads();
    for (int n = 0; n + 1 < N; ++n) {
        const size_t row = (size_t)r0 + n + 1;
        const double g_next = g[row], d_next = d[row];
        double Va_next = -INFINITY;
        if (has_absent) {
            // the first maximum of V[a][b] - switch over the valid pairs in row-major order, then the absent state
            double bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int i = t; i < SS; i += THREADS) {
                const int a = i / S, b = i - a * S;
                if (b - a >= mc) {
                    const double cand = m.A[i] - sw;
                    if (cand > bv) {
                        bv = cand;
                        bi = i;
                    }
                }
            }
            block_first_max(bv, bi, m.redv, m.redi);
            if (Va > bv) {
                bv = Va;
                bi = SS;
            }
            Va_next = absent_score[row] + bv;
            if (t == 0) back_absent[row] = bi;
        }
        for (int k = t; k < 2 * S - 1; k += THREADS) m.Tab[k] = gn * fabs(dn - (double)(k - (S - 1)) * dz);
        load_rows(m, S, score_top, score_base, row);
        __syncthreads();                                                    // the table, the next scores and V_n are whole
        unsigned char* b1 = back1 + row * (size_t)SS;
        pass_rows<false>(m.A, m.Tab, q, 1, [&](int x, int c, double v, int arg) {
            m.B[x * S + c] = v;
            b1[x * S + c] = (unsigned char)arg;
        });
        __syncthreads();                                                    // M1 is whole; V_n is free
        const double via = Va - sw;
        unsigned char* b2 = back2 + row * (size_t)SS;
        pass_cols<false>(m.B, m.Tab, q, 1, [&](int x, int c, double v, int arg) {
            if (has_absent && via > v) {
                v = via;
                arg = S;
            }
            m.A[x * S + c] = c - x >= mc ? node_score(m, has_ts, x, c) + v : -INFINITY;
            b2[x * S + c] = (unsigned char)arg;
        });
        __syncthreads();                                                    // V_{n+1} is whole; M1, the table and the scores are free
        Va = Va_next;
        gn = g_next;
        dn = d_next;
    }
    // the end of the path: the first maximum of the last V in row-major order, then the absent state
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = t; i < SS; i += THREADS) {
        const int a = i / S, b = i - a * S;
        if (b - a >= mc && m.A[i] > bv) {
            bv = m.A[i];
            bi = i;
        }
    }
    block_first_max(bv, bi, m.redv, m.redi);
    if (has_absent && Va > bv) {
        bv = Va;
        bi = SS;
    }
    // the path back, by one lane: the pointers stay on the device
    __threadfence();
    __syncthreads();
    if (t == 0) {
        __threadfence();
        log_score[blockIdx.x] = bv;
        int cur = bi;
        for (int n = N - 1; n >= 0; --n) {
            const size_t row = (size_t)r0 + n;
            const int a = cur / S, b = cur - a * S;
            cell_top[row] = cur == SS ? S : a;
            cell_base[row] = cur == SS ? S : b;
            if (n > 0) {
                if (cur == SS) {
                    cur = back_absent[row];
                } else {
                    const int pb = (int)back2[row * (size_t)SS + a * S + b];
                    cur = pb == S ? SS : (int)back1[row * (size_t)SS + a * S + pb] * S + pb;
                }
            }
        }
    }
}

// Scaled forward-backward over the pairs.  Forward: alpha_n (normalised) goes to the workspace row n and s_n to scale[n].  Backward:
// A holds u = w_{n+1} o beta_{n+1}; the two passes with the mirrored table give beta_n; gamma_n = alpha_n o beta_n goes to B, from
// which the three projections are summed, and A takes u = w_n o beta_n for the step before.  A thread reads back the alpha it wrote
// itself (the flat passes share one ownership, i = t + 512 j).
__global__ __launch_bounds__(THREADS) void k_unit_marginals(const long long* __restrict__ ptr, int S, int mc, int has_absent, int has_ts, double dz,
                                                            const double* __restrict__ score_top, const double* __restrict__ score_base,
                                                            const double* __restrict__ thickness_score, const double* __restrict__ absent_score,
                                                            const double* __restrict__ g, const double* __restrict__ d, double sw,
                                                            double* __restrict__ alpha, double* __restrict__ m_top, double* __restrict__ m_base,
                                                            double* __restrict__ m_thick, double* __restrict__ m_absent,
                                                            double* __restrict__ log_partition, double* __restrict__ scale)
{
    extern __shared__ double lds[];
    const int t = (int)threadIdx.x, SS = S * S;
    const size_t AW = (size_t)SS + 1;
    const Lds m(lds, S);
    const long long r0 = ptr[blockIdx.x];
    const int N = (int)(ptr[blockIdx.x + 1] - r0);
    if (N <= 0) {
        if (t == 0) log_partition[blockIdx.x] = 0.0;
        return;
    }
    const Geom q(S, mc);
    const double ks = exp(-sw);
    load_rows(m, S, score_top, score_base, (size_t)r0);
    if (has_ts)
        for (int k = t; k < S; k += THREADS) m.TS[k] = thickness_score[k];
    __syncthreads();
    // alpha_0 = w_0 / s_0
    double part = 0.0;
    for (int i = t; i < SS; i += THREADS) {
        const int a = i / S, b = i - a * S;
        const double u = b - a >= mc ? exp(node_score(m, has_ts, a, b)) : 0.0;
        m.A[i] = u;
        part += u;
    }
    double ua = has_absent ? exp(absent_score[r0]) : 0.0;
    double s = block_sum(part, m.redv) + ua;
    double lp = log(s);
    for (int i = t; i < SS; i += THREADS) {
        const double a = m.A[i] / s;
        m.A[i] = a;
        alpha[(size_t)r0 * AW + i] = a;
    }
    double aa = ua / s;
    if (t == 0) {
        alpha[(size_t)r0 * AW + SS] = aa;
        scale[r0] = s;
    }
    double gn = g[r0], dn = d[r0];
    __syncthreads();
    for (int n = 0; n + 1 < N; ++n) {
        const size_t row = (size_t)r0 + n + 1;
        const double g_next = g[row], d_next = d[row];
        double to_absent = 0.0;
        if (has_absent) {                                                   // sum over the valid pairs of alpha_n ks
            part = 0.0;
            for (int i = t; i < SS; i += THREADS) {
                const int a = i / S, b = i - a * S;
                if (b - a >= mc) part += m.A[i] * ks;
            }
            to_absent = block_sum(part, m.redv);
        }
        for (int k = t; k < 2 * S - 1; k += THREADS) m.Tab[k] = exp(-(gn * fabs(dn - (double)(k - (S - 1)) * dz)));
        load_rows(m, S, score_top, score_base, row);
        __syncthreads();                                                    // K, the next scores and alpha_n are whole
        pass_rows<true>(m.A, m.Tab, q, 1, [&](int x, int c, double v, int) { m.B[x * S + c] = v; });
        __syncthreads();
        const double from_absent = aa * ks;
        part = 0.0;
        pass_cols<true>(m.B, m.Tab, q, 1, [&](int x, int c, double v, int) {
            if (has_absent) v = v + from_absent;
            const double u = c - x >= mc ? exp(node_score(m, has_ts, x, c)) * v : 0.0;
            m.A[x * S + c] = u;
            part += u;
        });
        ua = has_absent ? exp(absent_score[row]) * (to_absent + aa) : 0.0;
        s = block_sum(part, m.redv) + ua;                                   // (its barriers: u is whole; the table and the scores are free)
        lp += log(s);
        for (int i = t; i < SS; i += THREADS) {
            const int a = i / S, b = i - a * S;
            double v = 0.0;
            if (b - a >= mc) {
                v = m.A[i] / s;
                m.A[i] = v;
            }
            alpha[row * AW + i] = v;
        }
        aa = ua / s;
        if (t == 0) {
            alpha[row * AW + SS] = aa;
            scale[row] = s;
        }
        gn = g_next;
        dn = d_next;
        __syncthreads();                                                    // alpha_{n+1} is whole
    }
    if (t == 0) log_partition[blockIdx.x] = lp;
    // backward: every thread reads the scale and the absent state's alpha its first lane wrote
    __threadfence();
    __syncthreads();
    __threadfence();
    double beta_a = 1.0, u_absent = 0.0, to_absent = 0.0;                   // u_absent = w_{n+1}[absent] beta_{n+1}[absent]; to_absent = sum ks u
    const int lane = t & 63, wave = t >> 6;
    for (int n = N - 1; n >= 0; --n) {
        const size_t row = (size_t)r0 + n;
        const bool last = n + 1 == N;
        load_rows(m, S, score_top, score_base, row);
        if (!last) {
            const double s_next = scale[row + 1];
            gn = g[row];
            dn = d[row];
            for (int k = t; k < 2 * S - 1; k += THREADS) m.Tab[k] = exp(-(gn * fabs(dn - (double)(k - (S - 1)) * dz)));
            __syncthreads();                                                // K and u are whole
            pass_rows<true>(m.A, m.Tab, q, -1, [&](int x, int c, double v, int) { m.B[x * S + c] = v; });
            __syncthreads();
            const double from_absent = ks * u_absent;
            pass_cols<true>(m.B, m.Tab, q, -1, [&](int x, int c, double v, int) {
                if (has_absent) v = v + from_absent;
                m.A[x * S + c] = v / s_next;
            });
            beta_a = has_absent ? (to_absent + u_absent) / s_next : 0.0;
        }
        __syncthreads();                                                    // beta_n and the scores of row n are whole; B is free
        double tot = 0.0, kb = 0.0;
        for (int i = t; i < SS; i += THREADS) {
            const int a = i / S, b = i - a * S;
            double gm = 0.0, u = 0.0;
            if (b - a >= mc) {
                const double beta = last ? 1.0 : m.A[i];
                gm = alpha[row * AW + i] * beta;
                u = exp(node_score(m, has_ts, a, b)) * beta;
            }
            m.B[i] = gm;
            m.A[i] = u;
            tot += gm;
            kb += ks * u;
        }
        const double gma = has_absent ? alpha[row * AW + SS] * beta_a : 0.0;
        u_absent = has_absent ? exp(absent_score[row]) * beta_a : 0.0;
        tot = block_sum(tot, m.redv) + gma;
        to_absent = block_sum(kb, m.redv);                                  // (gamma_n and u are whole)
        // the projections of gamma_n: base and thickness by columns (the row groups' partial sums meet in LDS), top by waves
        double pb = 0.0, pk = 0.0;
        for (int a = q.r; a < S; a += q.R) {
            pb += m.B[a * S + q.cc];
            if (a + q.cc < S) pk += m.B[a * S + a + q.cc];
        }
        m.part[t] = pb;
        m.part[THREADS + t] = pk;
        for (int a = wave; a < S; a += WAVES) {
            double v = (lane < S ? m.B[a * S + lane] : 0.0) + (lane + 64 < S ? m.B[a * S + lane + 64] : 0.0);
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) m_top[row * S + a] = v / tot;
        }
        __syncthreads();
        if (t < S) {
            const int BW = THREADS / q.R;
            double vb = m.part[t], vk = m.part[THREADS + t];
            for (int r = 1; r < q.R; ++r) {
                vb += m.part[r * BW + t];
                vk += m.part[THREADS + r * BW + t];
            }
            m_base[row * S + t] = vb / tot;
            m_thick[row * S + t] = vk / tot;
        }
        if (t == 0) m_absent[row] = gma / tot;
        __syncthreads();                                                    // the partial sums and B are free
    }
}

}  // namespace horizon_unit
