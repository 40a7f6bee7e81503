// A regularly spaced series and where it comes from: what the kernels on a kept ensemble share (included by
// gbp_ensemble.h, gbp_ensemble_diag.h and gbp_ensemble_corr.h).  Sounding b has n_rows rows of V variables; the used rows are seg_m[b]
// segments of seg_n[b] rows each that start at seg_start[b, :].  A row comes from one of two sources:
//   SERIES_PLAIN    x[b, t, v] (f64 [B, n_rows, V], v contiguous)
//   SERIES_RASTER   row t is slot t of the ensemble (ens_k [B, n_rows], ens_edges / ens_sigma [B, n_rows, K]) and variable v the depth-cell
//                   centre z[v]: the value of the layer that holds it, layer = #{l < k - 1 : edges[l] <= z} -- the hit map's own count,
//                   so an interface exactly at a centre gives the layer below.  [B, n_rows, V] never exists.
// THE RASTER RULE, once: a wave holds a slot's k - 1 edges (then +inf) and its k values (then NaN) one per lane (K <= 64; k clamped to
// 0 .. K), read once per row (slot_load); edge l is broadcast from its lane once and compared with every centre a lane holds, and the
// value comes from the lane that holds the layer -- two 32-bit halves, never through arithmetic (layers).  k == 0: NaN in every lane.
#pragma once
#include <hip/hip_runtime.h>

namespace ensemble {

enum { SERIES_PLAIN = 0, SERIES_RASTER = 1 };
constexpr int SERIES_MAX_M = 16;

struct SeriesArgs {                   // (the kernels' argument bytes: the order decides their code)
    int n_rows, V;                    // rows per sounding (PLAIN: of x; RASTER: slots), variables (RASTER: depth cells)
    const double* x;                  // PLAIN
    int K;                            // RASTER, and the four that follow
    const int* ens_k;
    const double* ens_edges;
    const double* ens_sigma;
    const double* z;
    int M_max, reach;                 // <= SERIES_MAX_M; the kernel's own extent: the largest lag (diagnostics), the band width W (correlation)
    const int* seg_start;             // [B, M_max]
    const int* seg_m;                 // [B]
    const int* seg_n;                 // [B]
};

struct Slot { int k, e_lo, e_hi; double s; };

// Slot src of the ensemble, one entry per lane; LOG10: the log10 of the stored values instead of the doubles.  !filled: as k == 0.
template <bool LOG10>
__device__ __forceinline__ Slot slot_load(const int* ens_k, const double* ens_edges, const double* ens_sigma, int K, size_t src, bool filled, int lane)
{
    Slot q;
    q.k = __builtin_amdgcn_readfirstlane(filled ? min(max(ens_k[src], 0), K) : 0);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double e = lane < q.k - 1 ? ens_edges[src * K + lane] : (double)INFINITY;
    q.s = lane < q.k ? (LOG10 ? log10(ens_sigma[src * K + lane]) : ens_sigma[src * K + lane]) : qnan;
    q.e_lo = __double2loint(e);
    q.e_hi = __double2hiint(e);
    return q;
}

// a row of a RASTER series: the slot's log10 conductivities
__device__ __forceinline__ Slot slot_load(const SeriesArgs& a, size_t src, int lane)
{
    return slot_load<true>(a.ens_k, a.ens_edges, a.ens_sigma, a.K, src, true, lane);
}

// x[g] = the slot's value at centre zc[g], g < G: G centres per lane at once (one readlane pair per edge serves them all)
template <int G>
__device__ __forceinline__ void layers(const Slot& q, const double* zc, double* x)
{
    int layer[G];
#pragma unroll
    for (int g = 0; g < G; ++g) layer[g] = 0;
    for (int l = 0; l < q.k - 1; ++l) {
        const double el = __hiloint2double(__builtin_amdgcn_readlane(q.e_hi, l), __builtin_amdgcn_readlane(q.e_lo, l));
#pragma unroll
        for (int g = 0; g < G; ++g) layer[g] += el <= zc[g] ? 1 : 0;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) x[g] = __shfl(q.s, layer[g], 64);
}

// Row `row` of sounding b among all rows, kept inside the sounding (a segment outside the rows is the caller's error: never a fault).
__device__ __forceinline__ size_t series_row(const SeriesArgs& a, size_t b, int row)
{
    return b * a.n_rows + (size_t)min(max(row, 0), a.n_rows - 1);
}

// The used rows of sounding b: M segments of N rows (wave-uniform); segment m starts at row series_starts(a, b)[m].
struct Segments { int M, N; };

__device__ __forceinline__ Segments series_segments(const SeriesArgs& a, size_t b)
{
    return {__builtin_amdgcn_readfirstlane(min(a.seg_m[b], a.M_max)), __builtin_amdgcn_readfirstlane(a.seg_n[b])};
}

__device__ __forceinline__ const int* series_starts(const SeriesArgs& a, size_t b) { return a.seg_start + b * a.M_max; }

}  // namespace ensemble
