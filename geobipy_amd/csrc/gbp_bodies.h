// Connected bodies of a realisation's raster (geobipy_amd/bodies.py label_reference states the rule in numpy;
// include/geobipy_amd.h gbp_bodies_label).  Nodes are the cells (s, c) of a raster [S, C]; a cell is a member iff lo <= v <= hi; cells
// are adjacent along a sounding ((s, c) - (s, c + 1)) and across an edge of the survey graph at the same column ((u, c) - (v, c)).
// The label of a member is the smallest linear index s C + c of its body, -1 for a non-member: canonical, so the device is held to
// the rule with ==.
//
//   k_bodies_label   one 1024-thread workgroup per (realisation, group); a group is a contiguous range of soundings that no edge
//                    leaves, and the edges are sorted by group, so a workgroup finds its own by two binary searches.  No word a
//                    workgroup writes is read by another one in the launch: nothing here depends on visibility across workgroups.
//     1 columns      a wave walks a sounding in chunks of 64 cells, lane = cell: two compares, one 64-bit ballot, and the top cell of
//                    the lane's run from the bits below it (carried across chunks).  label = s C + c_top: the vertical edges are done.
//     2 merging      a wave takes an edge, lane = cell: where both cells are members and the overlap of the two runs begins (c == 0
//                    or not both members at c - 1, from the ballot and a carried bit), the lane chases both cells to their roots and
//                    hooks the larger root onto the smaller with atomicMin; what the atomic returns says whether the larger one was
//                    still a root, and if it was not the lane goes on with the value it held (the loop of Playne and Hawick: the
//                    larger of the pair falls with every turn).  Then one step of pointer jumping.  Repeated until a sweep's hooks
//                    lower nothing; the labels only fall, so every loop is bounded by the node count.
//     3 flatten      every member cell to its root, and
//     4 accumulate   1 and q(s, c) = rint((a[s] t[c]) / unit) added at the root, after a sum over the lanes of the wave that share
//                    the root: integer atomics of one workgroup, exact in any order.
// Inside the workgroup a label another wave may have lowered is read only by an agent-scope relaxed atomic load and written only by an
// atomic: atomics execute in L2, and a plain load could be served from a line this CU's L1 already holds.  The flag that ends the
// sweeps lives in LDS between barriers and is set only from what an atomicMin returned (old > new).  No spin-wait, no grid barrier,
// no persistent wave; vector stores only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bodies {

constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_COLUMNS = 4096;
constexpr int MAX_REALISATIONS = 65536;

__device__ __forceinline__ int load_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_label(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int lower_label(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x: labels only fall and label[x] <= x, so the walk is at most as long as the node count.
__device__ __forceinline__ int find_root(const int* L, int x)
{
    int p = load_label(L + x);
    while (p != x) {
        x = p;
        p = load_label(L + x);
    }
    return x;
}

// The first e in 0 .. E with eu[e] >= s (eu's groups do not decrease along e).
__device__ __forceinline__ int first_edge_from(const int* __restrict__ eu, int E, long long s)
{
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (eu[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool MEASURE>
__global__ __launch_bounds__(THREADS) void k_bodies_label(int S, int C, int E, int G, const long long* __restrict__ group_ptr,
                                                          const int* __restrict__ eu, const int* __restrict__ ev,
                                                          const double* __restrict__ raster, double lo, double hi,
                                                          const double* __restrict__ a, const double* __restrict__ t, double unit,
                                                          int* __restrict__ label, int* __restrict__ cells,
                                                          long long* __restrict__ measure_q, int* __restrict__ sweeps)
{
    __shared__ int s_changed;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = (int)(blockIdx.x % (unsigned)G);
    const size_t r = blockIdx.x / (unsigned)G;
    const long long g0 = group_ptr[g], g1 = group_ptr[g + 1];
    if (g0 < 0 || g1 > S || g1 <= g0) {                                     // an empty group (the entry has refused the rest)
        if (tid == 0) sweeps[r * G + g] = 0;
        return;
    }
    const size_t base = r * (size_t)S * C;
    const double* const V = raster + base;
    int* const L = label + base;
    int* const N = cells + base;
    long long* const Q = MEASURE ? measure_q + base : nullptr;
    const int nodes = (int)(g1 - g0) * C;                                   // (R S C < 2^31)
    const unsigned long long below = (1ull << lane) - 1ull;

    // 1 columns
    for (int s = (int)g0 + wave; s < (int)g1; s += WAVES) {
        bool carried = false;                                               // the chunk before ended inside a run ...
        int carried_top = 0;                                                // ... that began here
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int c = c0 + lane;
            const bool in = c < C;
            const double v = in ? V[(size_t)s * C + c] : 0.0;
            const bool member = in && lo <= v && v <= hi;
            const unsigned long long m = __ballot(member);
            const unsigned long long out_below = ~m & below;
            const int top = out_below ? c0 + 64 - __clzll((long long)out_below) : (carried ? carried_top : c0);
            if (in) {
                const int at = s * C + c;
                store_label(L + at, member ? s * C + top : -1);
                N[at] = 0;
                if (MEASURE) Q[at] = 0;
            }
            if (m >> 63) {
                if (~m) {
                    carried_top = c0 + 64 - __clzll((long long)~m);
                } else if (!carried) {
                    carried_top = c0;
                }
                carried = true;
            } else {
                carried = false;
            }
        }
    }
    __threadfence();
    __syncthreads();

    // 2 merging
    const int e0 = first_edge_from(eu, E, g0), e1 = first_edge_from(eu, E, g1);
    int n_sweeps = 0;
    while (e1 > e0 && n_sweeps < nodes) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        bool lowered = false;
        for (int e = e0 + wave; e < e1; e += WAVES) {
            const long long u = eu[e], w = ev[e];
            if (u < g0 || u >= g1 || w < g0 || w >= g1 || u == w) continue;  // (never followed; the entry has refused them)
            bool both_before = false;                                       // both cells members at the last cell of the chunk before
            for (int c0 = 0; c0 < C; c0 += 64) {
                const int c = c0 + lane;
                const bool in = c < C;
                const int iu = (int)u * C + c, iw = (int)w * C + c;
                const bool both = in && load_label(L + iu) >= 0 && load_label(L + iw) >= 0;
                const unsigned long long m = __ballot(both);
                if (both && !(((m << 1) | (both_before ? 1ull : 0ull)) >> lane & 1ull)) {
                    int x = find_root(L, iu), y = find_root(L, iw);
                    while (x != y) {
                        if (x < y) {
                            const int z = x;
                            x = y;
                            y = z;
                        }
                        const int old = lower_label(L + x, y);              // x > y
                        lowered = lowered || old > y;
                        if (old == x) break;                                // x was a root: hooked
                        x = old;                                            // x hung below old: old and y are one body too
                    }
                }
                both_before = (m >> 63) != 0;
            }
        }
        if (__any(lowered) && lane == 0) s_changed = 1;
        __threadfence();
        __syncthreads();
        ++n_sweeps;
        const bool again = s_changed != 0;
        __syncthreads();
        if (!again) break;
        for (int i = tid; i < nodes; i += THREADS) {                        // pointer jumping: label[v] <- label[label[v]]
            const int at = (int)g0 * C + i;
            const int p = load_label(L + at);
            if (p >= 0 && p != at) {
                const int pp = load_label(L + p);
                if (pp < p) lower_label(L + at, pp);
            }
        }
        __threadfence();
        __syncthreads();
    }
    if (tid == 0) sweeps[r * G + g] = n_sweeps;

    // 3 flatten, 4 accumulate: a root's label is final now, and cells / measure_q are only added to
    for (int s = (int)g0 + wave; s < (int)g1; s += WAVES) {
        const double as = MEASURE ? a[s] : 0.0;
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int c = c0 + lane;
            const bool in = c < C;
            const int at = s * C + c;
            const int p = in ? load_label(L + at) : -1;
            const bool member = p >= 0;
            int root = -1;
            long long q = 0;
            if (member) {
                root = find_root(L, p);
                if (root != p) store_label(L + at, root);
                if (MEASURE) q = llrint((as * t[c]) / unit);
            }
            unsigned long long left = __ballot(member);
            while (left) {                                                  // one pair of atomics per root among the wave's cells
                const int first = __ffsll((unsigned long long)left) - 1;
                const int r0 = __shfl(root, first, 64);
                const bool same = member && root == r0;
                const unsigned long long m = __ballot(same);
                const long long qs = MEASURE ? wave_sum(same ? q : 0) : 0;
                if (lane == first) {
                    atomicAdd(N + r0, __popcll(m));
                    if (MEASURE) atomicAdd((unsigned long long*)(Q + r0), (unsigned long long)qs);
                }
                left &= ~m;
            }
        }
    }
}

}  // namespace bodies
