// Elevation slices: per-sounding columns on the DEPTH-below-surface axis resampled onto a shared ELEVATION axis, the reference's
// `Inference2D.elevationSlice(elevation, values)` (inversion/Inference2D.py:881-922) for every sounding and every elevation at once.
//
//   k_elevation_resample<false>  level E:            d = z_s - E;  out = v[cell(d)] when e[0] < d < e[n] (both strict), else NaN.
//   k_elevation_resample<true>   interval (lo, hi):  d0 = z_s - lo, d1 = z_s - hi;  out = mean(v[cell(d1) .. cell(d0)]) when d1 < e[n] and
//                                d0 > e[0] (the interval only has to OVERLAP the mesh: what sticks out above the surface or below the
//                                last edge is clipped away), NaN otherwise and for an empty range.
//   cell(d) = clamp(upper_bound(e, d) - 1, 0, n - 1): searchsorted(side='right') - 1, clipped.
// Every comparison is false for a NaN surface, so such a sounding is NaN; NaN values propagate.
//
// The mean is sum / count with the sum in numpy's pairwise order, because that is what the reference's `mean` adds up and the tests pin
// its bits: fewer than 8 terms left to right from 0; up to 128 terms eight accumulators r[j] = a[j], r[j] += a[i + j] over whole groups
// of eight, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remaining terms left to right; beyond 128 terms split at n / 2
// rounded down to a multiple of 8, sum each half by the same rule and add the two.  The recursion is walked with a path word and one
// parked sum per level (eight levels: 8191 cells at most), kept in registers.
//
// Mapping: the lanes of a wave take 64 consecutive elevation columns of ONE row, a workgroup four rows.  Stores are contiguous
// (out [R, columns] row-major, the [N, C] layout gbp_sibson_apply reads), neighbouring lanes read neighbouring depth cells of the row,
// the depth edges sit in LDS, the search and the sum are per lane.  fp64, no FMA (the library's build flags), no atomics.
#pragma once

namespace elev {

constexpr int COLS = 64;               // elevation columns per wave: one per lane
constexpr int ROWS = 4;                // rows per workgroup: one per wave
constexpr int LEVELS = 8;              // parked sums of the pairwise walk
constexpr int MAX_DEPTH_CELLS = 8191;  // n + 1 edges in 64 KB of LDS; the walk is at most seven levels deep there

__device__ inline int cell_of(const double* e, int n, double d)
{
    int lo = 0, hi = n + 1;            // the first edge above d
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] > d) hi = mid;
        else lo = mid + 1;
    }
    return min(max(lo - 1, 0), n - 1);
}

// at most 128 terms
__device__ inline double block_sum(const double* __restrict__ a, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        const double t0 = a[i], t1 = a[i + 1], t2 = a[i + 2], t3 = a[i + 3], t4 = a[i + 4], t5 = a[i + 5], t6 = a[i + 6], t7 = a[i + 7];
        r0 += t0; r1 += t1; r2 += t2; r3 += t3; r4 += t4; r5 += t5; r6 += t6; r7 += t7;
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

__device__ inline int half_of(int len)
{
    const int h = len / 2;
    return h - (h % 8);
}

__device__ inline double pairwise_sum(const double* __restrict__ a, int n)
{
    if (n <= 128) return block_sum(a, n);
    double parked[LEVELS];
#pragma unroll
    for (int k = 0; k < LEVELS; ++k) parked[k] = 0.0;
    int depth = 0;
    unsigned path = 0;                 // bit k: the right child at level k
    for (;;) {
        int off = 0, len = n;
        for (int k = 0; k < depth; ++k) {
            const int h = half_of(len);
            if ((path >> k) & 1u) {
                off += h;
                len -= h;
            } else
                len = h;
        }
        while (len > 128) {            // down the left side to a block
            len = half_of(len);
            path &= ~(1u << depth);
            ++depth;
        }
        double s = block_sum(a + off, len);
        while (depth > 0 && ((path >> (depth - 1)) & 1u)) {   // a right child closes its parent: left + right
            --depth;
            double left = 0.0;
#pragma unroll
            for (int k = 0; k < LEVELS; ++k) left = (k == depth) ? parked[k] : left;
            s = left + s;
        }
        if (depth == 0) return s;
#pragma unroll
        for (int k = 0; k < LEVELS; ++k) parked[k] = (k == depth - 1) ? s : parked[k];
        path |= 1u << (depth - 1);     // on to the right sibling
    }
}

// Workgroup (blockIdx.x, blockIdx.y): rows 4 blockIdx.x .. + 3 (one per wave), columns c0 + 64 blockIdx.y .. + 63 (one per lane) of the
// elevation axis; out [R, ncols] holds the window's columns only.  axis: levels [E] (INTERVAL = false) or edges [E + 1].
// Dynamic LDS: (n + 1) doubles.
template <bool INTERVAL>
__global__ __launch_bounds__(256) void k_elevation_resample(int R, int K, int n, const double* __restrict__ values,
                                                             const double* __restrict__ surface, const double* __restrict__ depth_edges,
                                                             const double* __restrict__ axis, int c0, int ncols, double* __restrict__ out)
{
    extern __shared__ double e[];
    for (int t = threadIdx.x; t <= n; t += 256) e[t] = depth_edges[t];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long r = (long long)blockIdx.x * ROWS + wave;
    const int c = blockIdx.y * COLS + lane;
    if (r >= R || c >= ncols) return;
    const double zs = surface[r / K];
    const double* v = values + (size_t)r * n;
    double res = __longlong_as_double(0x7ff8000000000000LL);
    if (!INTERVAL) {
        const double d = zs - axis[c0 + c];
        if (d > e[0] && d < e[n]) res = v[cell_of(e, n, d)];
    } else {
        const double d0 = zs - axis[c0 + c], d1 = zs - axis[c0 + c + 1];
        if (d1 < e[n] && d0 > e[0]) {
            const int first = cell_of(e, n, d1), last = cell_of(e, n, d0);
            if (first <= last) res = pairwise_sum(v + first, last - first + 1) / (double)(last - first + 1);
        }
    }
    out[(size_t)r * ncols + c] = res;
}

}  // namespace elev
