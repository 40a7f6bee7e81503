// Borehole logs as evidence for sections (the rule: include/geobipy_amd.h gbp_borehole_score and
// geobipy_amd/boreholes.py score_reference).  Included by gbp_fdem.hip after gbp_bodies.h.
//   k_borehole_score   the log weight every kept model of a sounding gets from the logs attached to it.  One wave per (sounding, 64
//                      models of its list), lane = model; the wave takes the sounding's attachments one after the other, so the sum
//                      over attachments has the rule's order without an atomic.  The 64 models are staged once in LDS -- per model the
//                      K - 1 interfaces (+inf past k - 1) and K values (log10 taken once per staged layer, NaN past k), a row of
//                      2 K - 1 doubles: an odd stride, as in the families kernels, so that the 64 lanes that read one pointer hit
//                      different bank pairs; a model has K - 1 interfaces and K values, so the row is already odd without the two
//                      sentinels of their 2 K + 1 (65 024 B of dynamic LDS at K = 64; two waves fit a compute unit's 160 KiB either
//                      way).  Interval data is the same for every lane: it is read once per
//                      interval, and every lane advances its own layer pointer through the ascending intervals, O(I + k) per lane and
//                      attachment.  The class posterior of a layer is kept until the lane's layer or the interval's class changes.
//                      The class constants of an attachment (ln pi - ln(v) / 2 and 2 v, v = scale^2 + var) are computed by the
//                      first C lanes into LDS.  A sounding without attachments gets zeros; the kernel writes every entry of score
//                      and part it owns.
// No atomics; every sum has one order, so a call repeats its own bits and identical models get identical bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace boreholes {

constexpr int WAVE = 64, MAX_MODELS = 1024, MAX_K = 64, MAX_CLASSES = 16;

__host__ __device__ constexpr int model_stride(int K) { return 2 * K - 1; }              // doubles per staged model
inline size_t lds_bytes(int K) { return (size_t)WAVE * model_stride(K) * sizeof(double); }      // 65 024 B at K = 64

struct ScoreArgs {
    int S, n_slots, K, n, C, chunks;  // chunks: waves per sounding, (n + 63) / 64
    const int* ens_k;
    const double* ens_edges;
    const double* ens_sigma;
    const int* rows;                  // [S, n]
    const int* n_used;                // [S]
    const int* att_ptr;               // [S + 1]
    const int* att_bore;              // [A]
    const double* att_var;            // [A]
    const double* att_shift;          // [A]
    const int* bore_ptr;              // [Nb + 1]
    const double* top;                // [I]
    const double* bottom;
    const double* value;
    const double* sd;
    const int* cls;                   // [I]: -1 measured, else the class
    double mean[MAX_CLASSES], scale[MAX_CLASSES], ln_prior[MAX_CLASSES];
    double floor;
    double* score;                    // [S, n]
    double* part;                     // [A, n] or NULL
    int* skipped;                     // [A] or NULL
};

// P(class c | a layer of value x) under the attachment's broadened classes: 1 / sum_q exp(l_q(x) - l_c(x)), q ascending.
__device__ __forceinline__ double class_posterior(double x, int c, int C, const double* mu, const double* cst, const double* two_v)
{
    const double dc = x - mu[c];
    const double lc = cst[c] - (dc * dc) / two_v[c];
    double sum = 0.0;
    for (int q = 0; q < C; ++q) {
        const double d = x - mu[q];
        const double lq = cst[q] - (d * d) / two_v[q];
        sum += exp(lq - lc);
    }
    return 1.0 / sum;
}

__global__ __launch_bounds__(WAVE) void k_borehole_score(ScoreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double bh_lds[];
    __shared__ double c_mu[MAX_CLASSES], c_cst[MAX_CLASSES], c_two_v[MAX_CLASSES];
    __shared__ int sk[WAVE];
    const int lane = threadIdx.x, K = a.K, n = a.n, C = a.C, St = model_stride(K);
    const size_t s = blockIdx.x / (unsigned)a.chunks;
    const int chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    const int m = chunk * WAVE + lane;
    const int a0 = a.att_ptr[s], a1 = a.att_ptr[s + 1];
    if (a0 >= a1) {                                                    // (the same for the whole wave: nobody waits at a barrier)
        if (m < n) a.score[s * n + m] = 0.0;
        return;
    }
    const int nu = min(max(a.n_used[s], 0), n);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    // ---- stage the wave's 64 models
    for (int idx = lane; idx < WAVE * K; idx += WAVE) {
        const int mm = idx / K, l = idx - mm * K;
        const int u = chunk * WAVE + mm;
        const int r = a.rows[s * n + min(u, n - 1)];
        const bool present = u < nu && r >= 0 && r < a.n_slots;
        const size_t src = s * a.n_slots + (size_t)min(max(r, 0), a.n_slots - 1);      // (clamped before any load)
        const int k = present ? min(max(a.ens_k[src], 0), K) : 0;
        if (l == 0) sk[mm] = k;
        double* const row = bh_lds + mm * St;
        if (l < K - 1) row[l] = l < k - 1 ? a.ens_edges[src * K + l] : (double)INFINITY;
        const double v = l < k ? a.ens_sigma[src * K + l] : qnan;
        row[K - 1 + l] = l < k ? log10(v) : v;
    }
    if (lane < C) c_mu[lane] = a.mean[lane];
    __syncthreads();

    const int k = sk[lane];
    const bool active = k > 0;
    const double* const row = bh_lds + lane * St;
    const double* const val = row + (K - 1);
    const double one_minus_floor = 1.0 - a.floor;
    double score = 0.0;
    for (int at = a0; at < a1; ++at) {
        const int b = a.att_bore[at];
        const double var = a.att_var[at], shift = a.att_shift[at];
        if (lane < C) {
            const double v = a.scale[lane] * a.scale[lane] + var;
            c_cst[lane] = a.ln_prior[lane] - 0.5 * log(v);
            c_two_v[lane] = 2.0 * v;
        }
        __syncthreads();
        double part = 0.0, held = 0.0;
        int skipped = 0, li = 0, held_layer = -1, held_class = -1;
        const int i0 = a.bore_ptr[b], i1 = a.bore_ptr[b + 1];
        for (int i = i0; i < i1; ++i) {                                // (uniform: every lane takes the same intervals)
            const double tp = fmax(a.top[i] + shift, 0.0), bp = a.bottom[i] + shift;
            if (bp <= tp) { ++skipped; continue; }                     // above the sounding's ground
            if (!active) continue;
            const int c = a.cls[i];
            const double h = bp - tp;
            while (li < k - 1 && row[li] <= tp) ++li;                  // (the count of interfaces <= t': they ascend, and so do the intervals)
            double p = tp, acc = 0.0;
            for (int step = 0; step < K + 1 && p < bp; ++step) {       // (at most k segments: the cap only guards malformed edges)
                const double ni = li < k - 1 ? row[li] : (double)INFINITY;
                const double q = fmin(ni, bp);
                double f;
                if (c < 0) f = val[li];
                else {
                    if (li != held_layer || c != held_class) {
                        held = class_posterior(val[li], c, C, c_mu, c_cst, c_two_v);
                        held_layer = li;
                        held_class = c;
                    }
                    f = held;
                }
                acc += (q - p) * f;
                li += ni == q ? 1 : 0;
                p = q;
            }
            const double mean = acc / h;
            double term;
            if (c < 0) {
                const double d = mean - a.value[i], e = a.sd[i];
                term = -(d * d) / (2.0 * (e * e + var));
            } else term = log(a.floor + one_minus_floor * mean);
            part += term;
        }
        if (m < n) {
            if (a.part) a.part[(size_t)at * n + m] = part;
            score += part;
        }
        if (a.skipped && chunk == 0 && lane == 0) a.skipped[at] = skipped;
        __syncthreads();                                               // (the class constants are written again)
    }
    if (m < n) a.score[s * n + m] = score;
}

}  // namespace boreholes
