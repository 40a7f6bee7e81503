// Survey volumes: discrete Sibson (natural-neighbour) gridding of per-sounding columns onto a regular x-y raster, the reference's
// `__sibson_2d_inner` (base/interpolation.py:57-89) split into a PLAN (geometry only, once per grid) and an APPLY (the hot gather,
// once per block of columns).  Pixel coordinates: sounding s sits at (px[s], py[s]) in units of pixels from the grid's first node.
//
//   k_grid_nearest   pixel (i, j) -> index = the nearest sounding to the NODE (j, i) (lowest index on a tie) and
//                    D = int(ceil(sqrt((j - px)^2 + (i - py)^2))), fp64, no FMA (the library's build flags), brute force with the
//                    soundings staged through LDS.
//   k_grid_segmax    the maximum of D over segments of 32 pixels of a row, and over whole rows: what prunes the walk below.
//   k_cover_walk     per DESTINATION pixel, the source pixels covering it, visited in row-major source order: source (i, j) covers
//                    (i_s, j_s) iff i - D <= i_s < i + D, j - D <= j_s < j + D and (i_s - i)^2 + (j_s - j)^2 <= D^2 + 0.25 (the upper
//                    bounds exclusive: a lopsided disc, nothing at D = 0).  Pass 1 counts (n), pass 2 writes index[source] into the
//                    destination's list.  A far pixel's disc reaches back to the survey, so no window bounds the walk: it visits
//                    every source row and skips the 32-pixel segments whose maximum D cannot reach.
//   k_sibson_gather  out[c, i_s, j_s] = (sum over the list, in list order, from 0.0, of values[list[p], c]) / n, NaN where the
//                    destination's own D^2 + 0.25 exceeds max_distance.  The lanes of a wave hold 64 consecutive columns of one
//                    row of `values` (512 contiguous bytes per load); the list entry is wave-uniform.  A workgroup owns 32
//                    destinations consecutive in x and 64 columns and transposes through LDS, so the stores run along x.
//   k_sibson_pool    pixel posteriors: pooled[i, v, c] = the sum over the list of pixel pixels[i] of the int32 hit maps
//                    maps[list[e], v - d_e, c], each neighbour's value axis moved by whole cells onto the nearest sounding's, and the
//                    counts that fell off the axis.  Integers: exact whatever the order.  Described at the kernel.
// The order of every sum is the list's order and nothing else: no atomics on the sums, no partial sums.
#pragma once

namespace grid {

constexpr int SEG = 32;        // pixels per pruning segment, and destinations per gather tile
constexpr int COLS = 64;       // columns per gather tile: one per lane
constexpr int STAGE = 1024;    // soundings per LDS stage of k_grid_nearest
constexpr int D_CAP = 1 << 30; // a D beyond any grid covers the whole raster: capped so that D * D stays inside int64

__global__ __launch_bounds__(256) void k_grid_nearest(int N, const double* __restrict__ px, const double* __restrict__ py, int nx, int ny,
                                                       int* __restrict__ index, int* __restrict__ D)
{
    __shared__ double sx[STAGE], sy[STAGE];
    const long long P = (long long)nx * ny;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = p < P;
    const double gi = live ? (double)(p / nx) : 0.0, gj = live ? (double)(p % nx) : 0.0;
    double best = 0.0;
    int who = -1;
    for (int s0 = 0; s0 < N; s0 += STAGE) {
        const int m = min(STAGE, N - s0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += 256) {
            sx[t] = px[s0 + t];
            sy[t] = py[s0 + t];
        }
        __syncthreads();
        for (int t = 0; t < m; ++t) {
            const double ax = gj - sx[t], ay = gi - sy[t];
            const double d2 = ax * ax + ay * ay;
            const bool take = who < 0 || d2 < best;       // (strict: the lowest index keeps a tie)
            best = take ? d2 : best;
            who = take ? s0 + t : who;
        }
    }
    if (live) {
        const double r = ceil(sqrt(best));
        index[p] = who;
        D[p] = r < (double)D_CAP ? (int)r : D_CAP;
    }
}

// segmax[i, s] = max D[i, 32 s .. 32 s + 31], rowmax[i] = max D[i, :]: one wave per row.
__global__ __launch_bounds__(64) void k_grid_segmax(int nx, int ny, int nseg, const int* __restrict__ D, int* __restrict__ segmax,
                                                    int* __restrict__ rowmax)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    int rm = 0;
    for (int s = lane; s < nseg; s += 64) {
        int m = 0;
        const int j1 = min(nx, (s + 1) * SEG);
        for (int j = s * SEG; j < j1; ++j) m = max(m, D[(size_t)i * nx + j]);
        segmax[(size_t)i * nseg + s] = m;
        rm = max(rm, m);
    }
    for (int o = 32; o > 0; o >>= 1) rm = max(rm, __shfl_xor(rm, o));
    if (lane == 0) rowmax[i] = rm;
}

// Destinations row0 * nx .. row1 * nx - 1, one thread each.  WRITE = false: n[dest] = the number of covering sources.
// WRITE = true: list[ptr[dest] - base + k] = index[k-th covering source in row-major order].
template <bool WRITE>
__global__ __launch_bounds__(256) void k_cover_walk(int nx, int ny, int nseg, int row0, int row1, const int* __restrict__ D,
                                                     const int* __restrict__ segmax, const int* __restrict__ rowmax,
                                                     const int* __restrict__ index, int* __restrict__ n, const long long* __restrict__ ptr,
                                                     long long base, int* __restrict__ list)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)(row1 - row0) * nx) return;
    const int is = row0 + (int)(q / nx), js = (int)(q % nx);
    const size_t dest = (size_t)is * nx + js;
    int count = 0;
    int* dst = WRITE ? list + (ptr[dest] - base) : nullptr;
    for (int i = 0; i < ny; ++i) {
        const int need_i = max(i - is, is - i + 1);        // i - D <= is < i + D
        if (rowmax[i] < need_i) continue;
        const long long di2 = (long long)(is - i) * (is - i);
        for (int s = 0; s < nseg; ++s) {
            const int j0 = s * SEG, j1 = min(nx, j0 + SEG);
            const int need_j = js < j0 ? j0 - js : (js >= j1 ? js - j1 + 2 : 1);
            if (segmax[(size_t)i * nseg + s] < max(need_i, need_j)) continue;
            for (int j = j0; j < j1; ++j) {
                const long long d = D[(size_t)i * nx + j];
                const long long dj = js - j;
                if (d >= need_i && d >= max(j - js, js - j + 1) && di2 + dj * dj <= d * d) {   // (integers: the + 0.25 admits nothing more)
                    if (WRITE) dst[count] = index[(size_t)i * nx + j];
                    ++count;
                }
            }
        }
    }
    if (!WRITE) n[dest] = count;
}

// Workgroup (blockIdx.x, blockIdx.y): tile order[tile0 + blockIdx.x] = 32 destinations of one row, columns 64 blockIdx.y .. + 63.
__global__ __launch_bounds__(256) void k_sibson_gather(int C, int nx, int ny, int tiles_per_row, const int* __restrict__ order, int tile0,
                                                        const long long* __restrict__ ptr, long long base, const int* __restrict__ list,
                                                        const int* __restrict__ D, double max_d2, const double* __restrict__ values,
                                                        double* __restrict__ out)
{
    __shared__ double tile[COLS][SEG + 1];
    const int t = order[tile0 + blockIdx.x];
    const int row = t / tiles_per_row, j0 = (t % tiles_per_row) * SEG, c0 = blockIdx.y * COLS;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double* col = values + min(c0 + lane, C - 1);    // (a lane past the last column reads the last one; it stores nothing)
    for (int q = wave; q < SEG && j0 + q < nx; q += 4) {
        const size_t dest = (size_t)row * nx + j0 + q;
        const long long p0 = ptr[dest] - base, p1 = ptr[dest + 1] - base;
        const int* l = list + p0;
        const long long len = p1 - p0;
        double acc = 0.0;
        constexpr int U = 8;                               // eight rows in flight per wave, added in list order
        long long k = 0;
        for (; k + U <= len; k += U) {
            double v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = col[(size_t)l[k + u] * C];
#pragma unroll
            for (int u = 0; u < U; ++u) acc += v[u];
        }
        for (; k < len; ++k) acc += col[(size_t)l[k] * C];
        const double d = (double)D[dest];
        tile[lane][q] = (d * d + 0.25 > max_d2) ? __longlong_as_double(0x7ff8000000000000LL) : acc / (double)len;
    }
    __syncthreads();
    const int d = threadIdx.x & (SEG - 1), g = threadIdx.x >> 5;
    if (j0 + d < nx) {
        const size_t P = (size_t)nx * ny, o = (size_t)row * nx + j0 + d;
#pragma unroll
        for (int c = g; c < COLS; c += 8)
            if (c0 + c < C) out[(size_t)(c0 + c) * P + o] = tile[c][d];
    }
}

// Pixel posteriors: the linear pool of the hit maps of a pixel's list, pooled[i, v, c] = sum over the entries e of maps[s_e, v - d_e, c],
// for the pixels of a caller's list (any order, repeats allowed).  d_e = (int) rint(u[s_e] - u[r]) clamped to +-n_value, r the pixel's
// nearest sounding (every sounding's value axis is centred on its own prior mean: u is that centre in value cells), 0 without u.
// clipped[i, c] = the counts of the rows that fell outside 0 <= v < n_value.  A masked pixel, an empty list and a pixel number outside
// the raster give zeros.  Integers only: the result does not depend on the order of anything.
//
// Workgroup blockIdx.x = i * tiles + t: pixel pixels[i], depth cells 64 CPL t .. + 64 CPL - 1, the depth tile fastest so that the
// workgroups in flight belong to few neighbouring pixels, which share most of their sources.  Lane l owns the cells c0 + 64 k + l,
// k < CPL: a (sounding, value row) load is CPL contiguous runs of 256 bytes.  The waves split the value rows in chunks of POOL_ROWS
// register accumulators and walk the list once per chunk; the entry and its shift are wave-uniform, and a chunk's loads of one entry
// are issued together (a row outside the axis is loaded from the nearest row inside and not added).  A lane past the last depth cell
// loads the last cell and stores nothing.  The last wave also sums the clipped rows, lane-local in int64.
constexpr int POOL_ROWS = 32;

__device__ __forceinline__ int pool_shift(const double* __restrict__ u, double ur, int s, int n_value)
{
    if (!u) return 0;
    const double t = rint(u[s] - ur), lim = (double)n_value;
    return __builtin_amdgcn_readfirstlane((int)fmin(fmax(t, -lim), lim));    // (wave-uniform: the row addresses stay scalar)
}

template <int CPL>
__global__ __launch_bounds__(256) void k_sibson_pool(int n_pixels, const int* __restrict__ pixels, int nx, int ny, int n_value, int n_depth,
                                                      int tiles, const long long* __restrict__ ptr, const int* __restrict__ list,
                                                      const int* __restrict__ index, const int* __restrict__ D, double max_d2,
                                                      const int* __restrict__ maps, const double* __restrict__ u, int* __restrict__ pooled,
                                                      long long* __restrict__ clipped)
{
    const int i = blockIdx.x / tiles, c0 = (blockIdx.x % tiles) * (64 * CPL);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = pixels[i];
    const int* l = list;
    long long len = 0;
    double ur = 0.0;
    if (p >= 0 && p < nx * ny) {
        const double d = (double)D[p];
        if (!(d * d + 0.25 > max_d2)) {
            l = list + ptr[p];
            len = ptr[p + 1] - ptr[p];
        }
        if (u) ur = u[index[p]];
    }
    unsigned c[CPL];
    bool live[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int cell = c0 + 64 * k + lane;
        live[k] = cell < n_depth;
        c[k] = 4u * (unsigned)min(cell, n_depth - 1);          // (bytes: a 32-bit lane offset beside a scalar row address)
    }
    const size_t map_cells = (size_t)n_value * n_depth, row_bytes = (size_t)n_depth * sizeof(int);
    for (int v0 = wave * POOL_ROWS; v0 < n_value; v0 += 4 * POOL_ROWS) {
        int acc[POOL_ROWS][CPL];
#pragma unroll
        for (int j = 0; j < POOL_ROWS; ++j)
#pragma unroll
            for (int k = 0; k < CPL; ++k) acc[j][k] = 0;
        for (long long e = 0; e < len; ++e) {
            const int s = l[e];
            const int lo = v0 - pool_shift(u, ur, s, n_value);            // the source row of the chunk's first row
            if (lo + POOL_ROWS <= 0 || lo >= n_value) continue;
            const int* m = maps + (size_t)s * map_cells;
            int val[POOL_ROWS][CPL];
            if (lo >= 0 && lo + POOL_ROWS <= n_value) {                  // every row inside the axis: addresses by increments
                const char* a[CPL];
#pragma unroll
                for (int k = 0; k < CPL; ++k) a[k] = (const char*)(m + (size_t)lo * n_depth) + c[k];
#pragma unroll
                for (int j = 0; j < POOL_ROWS; ++j)
#pragma unroll
                    for (int k = 0; k < CPL; ++k) {
                        val[j][k] = *(const int*)a[k];
                        a[k] += row_bytes;
                    }
#pragma unroll
                for (int j = 0; j < POOL_ROWS; ++j)
#pragma unroll
                    for (int k = 0; k < CPL; ++k) acc[j][k] += val[j][k];
                continue;
            }
#pragma unroll
            for (int j = 0; j < POOL_ROWS; ++j) {
                const int* row = m + (size_t)min(max(lo + j, 0), n_value - 1) * n_depth;
#pragma unroll
                for (int k = 0; k < CPL; ++k) val[j][k] = *(const int*)((const char*)row + c[k]);
            }
#pragma unroll
            for (int j = 0; j < POOL_ROWS; ++j) {
                const bool inside = lo + j >= 0 && lo + j < n_value;
#pragma unroll
                for (int k = 0; k < CPL; ++k) acc[j][k] += inside ? val[j][k] : 0;
            }
        }
        int* out = pooled + ((size_t)i * n_value + v0) * n_depth;
#pragma unroll
        for (int j = 0; j < POOL_ROWS; ++j)
            if (v0 + j < n_value) {
#pragma unroll
                for (int k = 0; k < CPL; ++k)
                    if (live[k]) *(int*)((char*)(out + (size_t)j * n_depth) + c[k]) = acc[j][k];
            }
    }
    if (wave == 3 && clipped) {
        long long lost[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) lost[k] = 0;
        if (u)
            for (long long e = 0; e < len; ++e) {
                const int s = l[e];
                const int d = pool_shift(u, ur, s, n_value);
                if (d == 0) continue;
                const int a = d > 0 ? n_value - d : 0, b = d > 0 ? n_value : -d;   // source rows a .. b - 1 land outside (|d| <= n_value)
                const int* m = maps + (size_t)s * map_cells;
                for (int v = a; v < b; ++v)
#pragma unroll
                    for (int k = 0; k < CPL; ++k) lost[k] += *(const int*)((const char*)(m + (size_t)v * n_depth) + c[k]);
            }
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if (live[k]) clipped[(size_t)i * n_depth + c[k] / 4] = lost[k];
    }
}

}  // namespace grid
