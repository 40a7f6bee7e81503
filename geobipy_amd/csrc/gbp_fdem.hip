// gbp_fdem.hip -- gfx950 kernels + C ABI (include/geobipy_amd.h) for the batched FDEM forward solve,
// Gaussian misfit / log-likelihood and Jacobian.  Hand-written for CDNA4 wave64; no CUDA path.
//
// Work decomposition:
//   workgroup  = one sounding  (NW waves; NW chosen on the host from the batch size)
//   wave       = one frequency at a time (f = wave, wave + NW, ...)
//   lane       = one Hankel abscissa: 64 abscissae per pass, 2 passes for the 120-point J0 filter
//   layer recursion, csqrt/cexp in registers; sigma / thickness of the sounding are wave-uniform
//   (scalar loads), the per-abscissa tables (40 B per point) are read coalesced from L2.
//   Hankel sum = wave64 butterfly reduction; chi^2 / logdet = second wave reduction over channels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/geobipy_amd.h"
#include "gbp_fdem_point.h"
#include "gbp_fdem_tables.h"

using gbp::Channel;
using gbp::cplx;

namespace {

thread_local char g_err[512] = "";

gbp_status fail(gbp_status code, const char* fmt, const char* detail = "")
{
    std::snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

#define GBP_HIP(call)                                                          \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) return fail(GBP_ERR_HIP, #call ": %s", hipGetErrorString(e_)); \
    } while (0)

}  // namespace

// Per-altitude-bin abscissa windows of one system (gbp_fdem_system_create_binned): bin i holds the tables windowed for soundings
// at altitude >= bin0 + i metres; the kernel picks a sounding's bin from its own altitude, so the terms that are evaluated for
// a sounding depend on that sounding only (never on the batch it is evaluated in).
struct BinDesc {
    int chan_off;        // first Channel of the bin in d_bin_chan
    int npts_total;      // points of the bin's flattened list (stride of its SoA)
    long long pts_off;   // first double of the bin's SoA in d_bin_pts
    int one_per_pass;    // 1: every frequency's window is exactly one 64-point pass, starting at 64 f (forward_passes_1f)
    int spare;
};

struct gbp_fdem_system {
    gbp::SystemTables t;      // host copy (channels, H0, point tables)
    Channel* d_chan = nullptr;
    double* d_pts = nullptr;  // SoA, GBP_PT_FIELDS arrays of [npts] (gbp_fdem_point.h)
    int bin0 = 0, n_bins = 0;
    // Further table sets of the same layout (gbp_hankel_system_add_set: e.g. the tables of other transmitter-receiver offsets);
    // row b of a launch uses set set_of_row[b], an ARGUMENT of the *_rows_ex entries (NULL: set 0) -- the handle holds no per-call
    // state, so host threads may share it.  Descriptor layout in d_bins: the n_bins altitude windows of set 0, then per further
    // set its full tables followed by its n_bins windows.
    std::vector<gbp::SystemTables> extra_sets;
    // host copies of every set's windowed tables for the current (eps, relative, first altitude, bin count): a handle that grows
    // set by set (gbp_tdem_forward meeting new receiver offsets) windows only the NEW sets in gbp_hankel_system_add_bins
    struct Pack {
        std::vector<BinDesc> desc;      // offsets relative to the pack's own chans / pts
        std::vector<Channel> chans;
        std::vector<double> pts;
    };
    std::vector<Pack> packs;
    double pack_eps = -1.0;
    int pack_relative = -1, pack_first = -1, pack_bins = -1;
    BinDesc* d_bins = nullptr;
    Channel* d_bin_chan = nullptr;
    double* d_bin_pts = nullptr;
    std::vector<int> bin_npts;
    // Soundings whose layers all have sigma >= sigma_direct take the kernels' csqrt_upper2<DIRECT> branch: for every
    // frequency f and abscissa with a = lambda^2 - omega^2 mu0 eps0 < 0,  -a <= wmu_f sigma / 4, i.e. b^2 >= 16 a^2.
    // (= 4 omega_max eps0, 2.9e-5 S/m at 130 kHz; 0 for tables without a displacement-current term)
    double sigma_direct = 0.0;
    void set_sigma_direct()
    {
        sigma_direct = 0.0;
        for (const Channel& ch : t.chan)
            for (int j = 0; j < ch.npts; ++j) {
                const double a = t.soa[(size_t)ch.off + j];   // field 0 of the SoA = a
                if (a < 0.0) sigma_direct = std::max(sigma_direct, -a / (0.25 * ch.wmu));
            }
    }
};

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
using namespace gbp;  // constants named by GBP_MATHK_INIT
__constant__ gbp::MathK GBP_K = GBP_MATHK_INIT;
__device__ const double GBP_EXP2_64[64] = GBP_EXP2_64_LIST;
__device__ const double GBP_SINCOS_64[128] = GBP_SINCOS_64_LIST;

// per-workgroup copy of the lookup tables in LDS + the scalar constants in SGPRs
struct MathLds {
    double exp2_64[64];
    gbp::SinCos sincos_64[64];
};
// SYNC = false: the caller's next workgroup barrier (the one behind the layer-thickness fill of forward_body / sens_body) is the tables'
// too -- the sampler's physics kernel fills them first thing, while its chain's move and layer count are still on their way
template <bool SYNC = true, bool ONE_WAVE = false>   // ONE_WAVE: the workgroup is one wave (lane i fills entry i)
__device__ __forceinline__ gbp::MathCtx math_setup(MathLds& lds)
{
    for (int i = threadIdx.x; i < 64; i += ONE_WAVE ? 64 : (int)blockDim.x) {
        lds.exp2_64[i] = GBP_EXP2_64[i];
        lds.sincos_64[i].s = GBP_SINCOS_64[2 * i];
        lds.sincos_64[i].c = GBP_SINCOS_64[2 * i + 1];
    }
    if (SYNC) __syncthreads();
    gbp::MathCtx M;
    M.k = GBP_K;
    M.e4_v = M.k.e4;
    M.s2_v = M.k.s2;
    M.c3_v = M.k.c3;
    asm volatile("" : "+v"(M.e4_v), "+v"(M.s2_v), "+v"(M.c3_v));  // opaque: stays in VGPRs, not re-materialised
    M.exp2_64 = lds.exp2_64;
    M.sincos_64 = lds.sincos_64;
    return M;
}

// Descriptor of (table set, altitude) in gbp_fdem_system::d_bins, or -1 for "the handle's own tables" (set 0 below the first bin).
__device__ __forceinline__ int table_slot(double alt, int set, int bin0, int n_bins)
{
    const bool binned = n_bins > 0 && alt >= (double)bin0;
    const int bi = binned ? min((int)(alt - (double)bin0), n_bins - 1) : 0;
    if (set == 0) return binned ? bi : -1;
    return n_bins + (set - 1) * (n_bins + 1) + (binned ? 1 + bi : 0);
}

// Sums over the 64 lanes by ONE balanced tree over the lane index (partners lane ^ 1, ^ 2, ^ 4, ... ^ 32): fp64 addition commutes,
// so every implementation of that tree below returns the same bits.
//   dpp_get<CTRL>: the value the DPP control names (VALU moves, no LDS crossbar round trip); lanes without a source read +0.0.
template <int CTRL>
__device__ __forceinline__ double dpp_get(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_mov_dpp((unsigned)u, CTRL, 0xf, 0xf, true);
    const unsigned hi = __builtin_amdgcn_mov_dpp((unsigned)(u >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_rows(double v)      // (masked-off rows add +0.0)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)u, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)(u >> 32), CTRL, ROW_MASK, 0xf, false);
    return v + __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// Sum of v, returned to every lane as a wave-uniform value.  Quad swaps, then row shifts by 4 and 8 (lanes 12 - 15 of a row hold the
// row's sum), then the previous row's lane 15 broadcast into rows 1 - 3 and lane 31 into rows 2 - 3: lane 63 holds the total.
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_get<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_get<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_get<0x114>(v);      // row_shr:4
    v += dpp_get<0x118>(v);      // row_shr:8
    v = dpp_add_rows<0x142, 0xa>(v);     // row_bcast:15 -> rows 1 and 3
    v = dpp_add_rows<0x143, 0xc>(v);     // row_bcast:31 -> rows 2 and 3: lane 63 holds the total
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, 63), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// This library is written for gfx950 alone (v_permlane16_swap / v_permlane32_swap below exist on no earlier CDNA part): say so at
// compile time rather than with an unknown-builtin error in the middle of the reduction tree.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "geobipy_amd builds for gfx950 (MI355X) only: hipcc --offload-arch=gfx950"
#endif
// v[lane] + v[lane ^ W] for W = 16, 32 in every lane, by gfx950's row swaps (v_permlane16_swap / v_permlane32_swap exchange the odd
// 16- / 32-lane rows of one register with the even rows of another: VALU moves, where a shuffle would wait for the LDS crossbar;
// ds_swizzle / ds_bpermute for every exchange of wave_sum_store2 and wave_sum_tail were measured in the VALU-bound headline kernel and
// were no faster, docs/notes_r9.md)
template <int W>
__device__ __forceinline__ void row_pair(double v, double& x, double& y)     // {x, y} = {v[lane], v[lane ^ W]} in some order
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    const auto a = W == 16 ? __builtin_amdgcn_permlane16_swap(lo, lo, false, false) : __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto b = W == 16 ? __builtin_amdgcn_permlane16_swap(hi, hi, false, false) : __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    x = __builtin_bit_cast(double, ((unsigned long long)b[0] << 32) | a[0]);
    y = __builtin_bit_cast(double, ((unsigned long long)b[1] << 32) | a[1]);
}
template <int W>
__device__ __forceinline__ double row_pair_sum(double v)
{
    double x, y;
    row_pair<W>(v, x, y);
    return x + y;
}
// Sums of a AND b with one tree instead of two: after the first exchange the even lanes carry a's partial sums and the odd lanes b's
// (the partner of an even lane sends its a, the partner of an odd lane its b), every later step pairs lanes of the same parity.
// Returns, in lane 62, the sum of a and, in lane 63, the sum of b -- the bits wave_sum(a) / wave_sum(b) return.  (The cross-row steps
// are row swaps: row_bcast only broadcasts lane 15, an odd one.)  26 VALU issues against 2 x 32.
__device__ __forceinline__ double wave_sum_pair(double a, double b, int lane)
{
    const bool odd = lane & 1;
    double v = odd ? b : a;
    v += dpp_get<0xB1>(odd ? a : b);
    v += dpp_get<0x4E>(v);
    v += dpp_get<0x114>(v);
    v += dpp_get<0x118>(v);
    v = row_pair_sum<16>(v);
    v = row_pair_sum<32>(v);
    return v;
}
// ... stored as one complex number (lanes 62 and 63 write their halves)
__device__ __forceinline__ void wave_sum_store(double re, double im, int lane, cplx* dst)
{
    const double v = wave_sum_pair(re, im, lane);
    if (lane >= 62) reinterpret_cast<double*>(dst)[lane - 62] = v;
}
// Two complex sums (a: re0, im0; b: re1, im1) with one tree, stored to dst[0] and dst[2] (the partials of two consecutive passes).  The
// lane ^ 1 step leaves the real parts of both in the even lanes and the imaginary parts in the odd ones, the lane ^ 2 step pass a in
// lanes 0, 1 of every quad and pass b in lanes 2, 3; from there on it is wave_sum_pair's tree.  Every value meets the partners it meets
// in wave_sum_store, in the same order: the same bits, for 37 VALU issues against 2 x 26.
__device__ __forceinline__ void wave_sum_store2(double re0, double im0, double re1, double im1, int lane, cplx* dst)
{
    const bool odd = lane & 1, hi = lane & 2;
    double x = odd ? im0 : re0, y = odd ? im1 : re1;
    x += dpp_get<0xB1>(odd ? re0 : im0);     // quad_perm [1,0,3,2]
    y += dpp_get<0xB1>(odd ? re1 : im1);
    double v = hi ? y : x;
    v += dpp_get<0x4E>(hi ? x : y);          // quad_perm [2,3,0,1]
    v += dpp_get<0x114>(v);
    v += dpp_get<0x118>(v);
    v = row_pair_sum<16>(v);
    v = row_pair_sum<32>(v);
    if (lane >= 60) reinterpret_cast<double*>(dst)[(lane & 3) + (lane & 2)] = v;   // lanes 60 - 63: re0, im0, re1, im1
}

// Smallest conductivity of the sounding (wave-uniform, returned in SGPRs; each wave of the workgroup evaluates it).
__device__ __forceinline__ double wave_min_sigma(const double* __restrict__ sig, int L, int lane)
{
    double v = 1.7976931348623157e308;
    for (int k = lane; k < L; k += 64) v = fmin(v, sig[k]);
    v = fmin(v, dpp_get<0xB1>(v));       // (a minimum does not depend on the order: quad swaps, the two mirrors of a row, row swaps)
    v = fmin(v, dpp_get<0x4E>(v));
    v = fmin(v, dpp_get<0x141>(v));
    v = fmin(v, dpp_get<0x140>(v));
    double x, y;
    row_pair<16>(v, x, y); v = fmin(x, y);
    row_pair<32>(v, x, y); v = fmin(x, y);
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Per-frequency layer constants of this sounding -> LDS (lanes k < L), then a wave barrier.
__device__ __forceinline__ void setup_layers(gbp::LayerK* lay, double wmu, const double* __restrict__ sig, int L,
                                             int lane)
{
    for (int k = lane; k < L; k += 64) {
        const double b = wmu * sig[k];
        lay[k].b2 = b * b;
        lay[k].bc = b * 0.70710678118654752440;
    }
    __builtin_amdgcn_wave_barrier();
}

// Forward solve over a contiguous range of 64-point passes of the sounding's FLATTENED (frequency, abscissa)
// point list (P points: 120 per zz frequency, 140 per xz/zx, 260 per xx).  Flattening matters because 120 is
// not a multiple of 64: per-frequency passes would idle 8 of 128 lanes, the flat list idles < 64 of P.
// A pass may straddle two frequencies ("cur" below the boundary lane, "next" above it; never three: a frequency has at
// least 64 points): each lane picks its frequency's layer constants (two LDS slots) and altitude term.
// Summation order: every pass reduces its lanes' terms -- per frequency -- to ONE partial sum, sh_part[p][0] for the
// frequency its first point belongs to and sh_part[p][1] for the one that starts inside it; forward_body adds a frequency's
// partials in pass order.  The result therefore does not depend on which wave ran which pass: any number of waves per
// sounding gives the same bits.
template <bool DIRECT>   // csqrt_upper2<DIRECT> is valid for every layer and abscissa of this sounding (gbp_fdem_system::sigma_direct)
__device__ __forceinline__ void forward_passes(const gbp::MathCtx& M, const Channel* __restrict__ chan,
                                               const double* __restrict__ pts, int P, int F, int L,
                                               const double* __restrict__ sig, const double* sh_t2,
                                               gbp::LayerK* sh_lay /* [2][Lmax] */, int Lmax, double alt, int p0,
                                               int p1, int lane, cplx* sh_part /* [npass][2] of the sounding */, double row_scale)
{
    if (p0 >= p1) return;
    int cur = 0;
    while (cur + 1 < F && chan[cur].off + chan[cur].npts <= 64 * p0) ++cur;
    int slot = 0;
    bool cur_ready = false;
    for (int p = p0; p < p1; ++p) {
        const Channel cc = chan[cur];
        if (!cur_ready) {
            setup_layers(sh_lay + (size_t)slot * Lmax, cc.wmu, sig, L, lane);
            cur_ready = true;
        }
        const int base = 64 * p;
        const int end_cur = cc.off + cc.npts;
        const bool has_next = (base + 64 > end_cur) && (cur + 1 < F);
        double hD = cc.hd0 - 2.0 * alt;
        const gbp::LayerK* lay = sh_lay + (size_t)slot * Lmax;
        int j = base + lane;
        const bool valid = j < P;
        bool in_next = false;
        if (has_next) {
            const Channel cn = chan[cur + 1];
            setup_layers(sh_lay + (size_t)(slot ^ 1) * Lmax, cn.wmu, sig, L, lane);
            in_next = j >= end_cur;
            if (in_next) {
                hD = cn.hd0 - 2.0 * alt;
                lay = sh_lay + (size_t)(slot ^ 1) * Lmax;
            }
        }
        gbp::Point pt;
        if (base + 64 > P) {   // ragged tail of the point list (wave-uniform branch)
            pt = gbp::load_point(pts, P, valid ? j : P - 1);
            if (!valid) pt.coef = gbp::mk(0.0, 0.0);
        } else {
            pt = gbp::load_point(pts, P, j);
        }
        if (row_scale != 1.0) gbp::scale_point(pt, row_scale);     // (wave-uniform: a receiver moved off its table set's distance)
        cplx num, den;
        gbp::rte_num_den<DIRECT>(M, pt.a, L, lay, sh_t2, pt.u0, num, den);
        const bool real_ue = __ballot(pt.ue.im != 0.0) == 0ull;            // (wave-uniform: see hankel_term)
        const cplx t = gbp::hankel_term(M, num, den, pt.ue, hD, pt.coef, real_ue);
        if (has_next) {
            wave_sum_store(in_next ? 0.0 : t.re, in_next ? 0.0 : t.im, lane, sh_part + 2 * p);
            wave_sum_store(in_next ? t.re : 0.0, in_next ? t.im : 0.0, lane, sh_part + 2 * p + 1);
        } else {
            wave_sum_store(t.re, t.im, lane, sh_part + 2 * p);
        }
        if (base + 64 >= end_cur) {   // frequency `cur` has no points beyond this pass
            ++cur;
            cur_ready = has_next;
            slot ^= 1;
            if (cur >= F) break;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// forward_passes for a table set whose every frequency is exactly one pass (BinDesc::one_per_pass: chan[f].off == 64 f, npts == 64):
// pass p is frequency p, so there is no frequency cursor, no second layer slot, no straddle and no ragged tail.  Each pair of passes
// goes through one reduction tree (wave_sum_store2); the partials are the ones forward_passes stores, bit for bit.  The plain forward
// kernel's path (no row scale).
// The wave's share of the layer tables is used as LayerRec rec[Lmax] here (the bytes of LayerK lay[2][Lmax]): -2 thk_k sits in layer k's
// record, written once per sounding, and the recursion reads the records from ONE base address held in a VGPR (rte_num_den_rec), where
// separate tables at run-time distances cost two address copies per layer.
typedef const __attribute__((address_space(3))) gbp::LayerRec* lds_rec_cp;
// gbp::hankel_term with the exponent clamped by ONE v_max_f64: the argument is a product, hence canonical already, which the compiler
// does not see through fmax (it puts a canonicalising v_max_f64 v, v in front).  The clamp's result is fmax's for every input, NaN included.
__device__ __forceinline__ double clamp_exp_arg(double x)
{
    double r;
    const double lo = -800.0;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "s"(lo));
    return r;
}
__device__ __forceinline__ cplx hankel_term_1f(const gbp::MathCtx& M, cplx num, cplx den, cplx ue, double hD, cplx coef, bool real_ue)
{
    const double x = clamp_exp_arg(ue.re * hD);
    if (real_ue) return gbp::cdiv(num * (coef * gbp::exp_neg_clamped(M, x)), den);
    const cplx E = gbp::cexp_neg_clamped(M, x, ue.im * hD);
    return gbp::cdiv(num * (E * coef), den);
}
template <bool DIRECT>
__device__ __forceinline__ void forward_passes_1f(const gbp::MathCtx& M, const Channel* __restrict__ chan,
                                                  const double* __restrict__ pts, int P, int L, const double* __restrict__ sig,
                                                  const double* __restrict__ th, gbp::LayerRec* sh_rec, double alt, int p0, int p1,
                                                  int lane, cplx* sh_part)
{
    cplx prev = gbp::mk(0.0, 0.0);
    // setup_layers for up to 64 layers (wave-uniform): lane k keeps sigma_k in a register for all passes and writes layer k's
    // constants with one predicated statement -- no loop, no pointer stepping, no load of sigma in every pass; the same products
    const bool lane_per_layer = L <= 64;
    const double sig_k = (lane_per_layer && lane < L) ? sig[lane] : 0.0;
    for (int k = lane; k < L - 1; k += 64) sh_rec[k].t2 = -2.0 * th[k];
    // the records' LDS address, opaque and in a VGPR: every ds_read of the recursion is this register plus an immediate
    unsigned rec_at = (unsigned)(size_t)(lds_rec_cp)sh_rec;
    asm volatile("" : "+v"(rec_at));
    const lds_rec_cp rec = (lds_rec_cp)(size_t)rec_at;
    for (int p = p0; p < p1; ++p) {
        const Channel cc = chan[p];
        if (lane_per_layer) {
            if (lane < L) {
                const double b = cc.wmu * sig_k;
                sh_rec[lane].b2 = b * b;
                sh_rec[lane].bc = b * 0.70710678118654752440;
            }
        } else {
            for (int k = lane; k < L; k += 64) {
                const double b = cc.wmu * sig[k];
                sh_rec[k].b2 = b * b;
                sh_rec[k].bc = b * 0.70710678118654752440;
            }
        }
        __builtin_amdgcn_wave_barrier();
        const double hD = cc.hd0 - 2.0 * alt;
        const gbp::Point pt = gbp::load_point_u(pts, P, (unsigned)(64 * p + lane));
        cplx num, den;
        gbp::rte_num_den_rec<DIRECT>(M, pt.a, L, rec, pt.u0, num, den);
        const bool real_ue = __ballot(pt.ue.im != 0.0) == 0ull;            // (wave-uniform: see hankel_term)
        const cplx t = hankel_term_1f(M, num, den, pt.ue, hD, pt.coef, real_ue);
        if ((p - p0) & 1)
            wave_sum_store2(prev.re, prev.im, t.re, t.im, lane, sh_part + 2 * (p - 1));
        else if (p + 1 == p1)
            wave_sum_store(t.re, t.im, lane, sh_part + 2 * p);
        prev = t;
        __builtin_amdgcn_wave_barrier();
    }
}

// chi^2 / logL of one sounding from N predicted channels held in `p` (LDS or global); executed by one wave.
__device__ __forceinline__ void loglike_wave(int N, const double* p, const double* __restrict__ obs, double rel,
                                             double add, int lane, double* chi2, double* logL)
{
    double s2 = 0.0, logdet = 0.0, na = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double o = obs[i];
        const bool active = o > 0.0;  // false for NaN and for non-positive data (EmDataPoint.py:54-56)
        const double ro = rel * o;
        const double var = ro * ro + add * add;  // DataPoint.py:274
        if (active) {
            const double r = (p[i] - o) * (1.0 / sqrt(var));  // DataPoint.py:523-524
            s2 += r * r;
            logdet += log(var);
            na += 1.0;
        }
    }
    // chi^2 and log-determinant share one reduction tree (lane 62 ends with chi^2, lane 63 with the log-determinant: the bits of two
    // wave_sums); the count of active channels -- a sum of ones, exact in any order -- goes through its own
    const double mine = wave_sum_pair(s2, logdet, lane);
    const double other = dpp_get<0xB1>(mine);
    na = wave_sum(na);
    if (lane == 62) *chi2 = mine;
    // MvNormalDistribution.py:209-216 with a diagonal covariance
    if (lane == 63) *logL = -(0.5 * na) * 1.8378770664093453 - 0.5 * mine - 0.5 * other;
}

// Sum of v by the tree wave_sum_pair runs on its first argument: lanes 60 - 63 return the bits lane 62 of wave_sum_pair(v, .) returns
// (there the even lanes carry v's partial sums from the first exchange on and meet even lanes only; here every lane does).
__device__ __forceinline__ double wave_sum_tail(double v)
{
    v += dpp_get<0xB1>(v);
    v += dpp_get<0x4E>(v);
    v += dpp_get<0x114>(v);
    v += dpp_get<0x118>(v);
    v = row_pair_sum<16>(v);
    v = row_pair_sum<32>(v);
    return v;
}

// loglike_wave with the terms that do not depend on the model prepared once per batch (k_gauss_prepare): w[i] = 1 / sqrt(var_i) of
// the active channels and c0 = -(0.5 na) ln 2pi - 0.5 logdet, the value loglike_wave holds before it subtracts 0.5 chi^2.  A channel is
// inactive by the rule of loglike_wave, read from the data themselves (the residual needs them anyway): its weight is never touched.
__device__ __forceinline__ void loglike_wave_prepared(int N, const double* p, const double* __restrict__ obs,
                                                      const double* __restrict__ w, const double* __restrict__ c0, int lane,
                                                      double* chi2, double* logL)
{
    double s2 = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double o = obs[i];
        if (o > 0.0) {
            const double r = (p[i] - o) * w[i];
            s2 += r * r;
        }
    }
    s2 = wave_sum_tail(s2);
    if (lane == 62) *chi2 = s2;
    if (lane == 63) *logL = *c0 - 0.5 * s2;
}

// Forward solve (+ chi^2 / logL) of ONE sounding by the calling workgroup: the body of k_fdem_forward, also called once per
// iteration by the persistent sampler kernel (gbp_rjmcmc.h).  Every thread of the workgroup must call it (it contains
// workgroup barriers); `sh_out` holds 2 * GBP_MAX_FREQ doubles, `sh_dyn` dyn_lds_bytes(nwaves, Lmax, passes) bytes:
//   LayerK lay[nwaves][2][Lmax] | cplx part[passes][2] | double t2[Lmax]
// (forward_passes_1f keeps LayerRec rec[nwaves][Lmax] in the bytes of `lay` and leaves `t2` alone)
// The passes are shared by the first `nw_use` waves of the workgroup (the others only take part in the barriers); the result
// does not depend on nw_use (see forward_passes).
// ONE_PER_PASS (the plain forward kernel): the table set's frequencies are one pass each when `one_per_pass` (BinDesc) is set, and
// forward_passes_1f runs them; the sampler's kernels instantiate the general path only.
// PREPARED (k_fdem_forward_prepared): the likelihood from prepared terms, `rel_b` / `add_b` unused, `w_row`, `c0_b` instead.
// ONE_WAVE (its one-wave-per-sounding instance): the workgroup IS one wave, known at compile time.
template <bool LIKE, bool ONE_PER_PASS = false, bool PREPARED = false, bool ONE_WAVE = false>
__device__ __forceinline__ void forward_body(const gbp::MathCtx& M, double* sh_out, unsigned char* sh_dyn,
                                             const Channel* __restrict__ chan, const double* __restrict__ pts, int npts_total,
                                             int F, int Lmax, int L, const double* __restrict__ sig,
                                             const double* __restrict__ th, double alt, const double* __restrict__ obs_row,
                                             double rel_b, double add_b, double* __restrict__ pred_row, double* chi2_b,
                                             double* logL_b, double sigma_direct, int nw_use, double row_scale = 1.0,
                                             bool one_per_pass = false, const double* __restrict__ w_row = nullptr,
                                             const double* __restrict__ c0_b = nullptr)
{
    const int lane = threadIdx.x & 63;
    const int wave = ONE_WAVE ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = ONE_WAVE ? 1 : nw_use;
    const unsigned tid = ONE_WAVE ? (unsigned)lane : threadIdx.x, nth = ONE_WAVE ? 64u : blockDim.x;
    const int npass = (npts_total + 63) >> 6;
    // every layer conductive enough for the select-free complex sqrt (all but displacement-current dominated models)
    const bool direct = wave_min_sigma(sig, L, lane) >= sigma_direct;   // workgroup-uniform
    gbp::LayerK* sh_lay = reinterpret_cast<gbp::LayerK*>(sh_dyn) + (size_t)wave * 2 * Lmax;
    cplx* sh_part = reinterpret_cast<cplx*>(sh_dyn + (size_t)nwaves * 2 * Lmax * sizeof(gbp::LayerK));
    double* sh_t2 = reinterpret_cast<double*>(sh_part + (size_t)2 * npass);
    const bool records = ONE_PER_PASS && one_per_pass;     // (workgroup-uniform: the sounding's own table set)
    if (!records)
        for (int k = tid; k < L - 1; k += nth) sh_t2[k] = -2.0 * th[k];
    __syncthreads();

    if (wave < nwaves) {
        const int per = (npass + nwaves - 1) / nwaves;
        const int p0 = wave * per;
        const int p1 = min(npass, p0 + per);
        if (records) {
            gbp::LayerRec* sh_rec = reinterpret_cast<gbp::LayerRec*>(sh_lay);
            if (direct)
                forward_passes_1f<true>(M, chan, pts, npts_total, L, sig, th, sh_rec, alt, p0, p1, lane, sh_part);
            else
                forward_passes_1f<false>(M, chan, pts, npts_total, L, sig, th, sh_rec, alt, p0, p1, lane, sh_part);
        } else if (direct) {
            forward_passes<true>(M, chan, pts, npts_total, F, L, sig, sh_t2, sh_lay, Lmax, alt, p0, p1, lane, sh_part, row_scale);
        } else {
            forward_passes<false>(M, chan, pts, npts_total, F, L, sig, sh_t2, sh_lay, Lmax, alt, p0, p1, lane, sh_part, row_scale);
        }
    }
    __syncthreads();

    // out_f = 1e6 * scale * (H - H0) / H0 = g_f * sum of the frequency's per-pass partials in pass order
    for (int f = tid; f < F; f += nth) {
        const Channel ch = chan[f];
        double sr = 0.0, si = 0.0;
        for (int p = ch.off >> 6; 64 * p < ch.off + ch.npts; ++p) {
            const cplx v = sh_part[2 * p + (64 * p >= ch.off ? 0 : 1)];   // the pass's own frequency, or the one starting inside it
            sr += v.re; si += v.im;
        }
        sh_out[f] = ch.g_re * sr - ch.g_im * si;
        sh_out[F + f] = ch.g_re * si + ch.g_im * sr;
    }
    __syncthreads();

    const int N = 2 * F;
    if (pred_row != nullptr)
        for (int i = tid; i < N; i += nth) pred_row[i] = sh_out[i];
    if (LIKE && wave == 0) {
        if (PREPARED)
            loglike_wave_prepared(N, sh_out, obs_row, w_row, c0_b, lane, chi2_b, logL_b);
        else
            loglike_wave(N, sh_out, obs_row, rel_b, add_b, lane, chi2_b, logL_b);
    }
}

template <bool LIKE, bool SCALED = false>   // SCALED: the rows carry a distance scale (gbp_fdem_forward_rows_scaled); the plain kernels do not pay for it (4 VGPRs, 36 B of scratch)
__global__ __launch_bounds__(1024) void k_fdem_forward(const Channel* __restrict__ chan,
                                                       const double* __restrict__ pts, int npts_total, int F,
                                                       int Lmax, const int* __restrict__ nlayers,
                                                       const double* __restrict__ sigma,
                                                       const double* __restrict__ thk,
                                                       const double* __restrict__ height,
                                                       const double* __restrict__ obs,
                                                       const double* __restrict__ rel,
                                                       const double* __restrict__ add, double* __restrict__ pred,
                                                       double* __restrict__ chi2, double* __restrict__ logL,
                                                       double sigma_direct, const BinDesc* __restrict__ bins, int bin0, int n_bins,
                                                       const Channel* __restrict__ bin_chan, const double* __restrict__ bin_pts,
                                                       const int* __restrict__ row_set, const double* __restrict__ row_scale)
{
    __shared__ double sh_out[2 * GBP_MAX_FREQ];
    __shared__ MathLds sh_math;
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_dyn[];
    const int b = blockIdx.x;
    bool one_per_pass = false;
    if (bins != nullptr) {                                  // this sounding's table set and abscissa window (the bin of its own altitude)
        const int slot = table_slot(height[b], row_set != nullptr ? row_set[b] : 0, bin0, n_bins);
        if (slot >= 0) {                                    // (set 0 below the first bin, NaN: the handle's own tables, all abscissae)
            const BinDesc d = bins[slot];
            chan = bin_chan + d.chan_off;
            pts = bin_pts + d.pts_off;
            npts_total = d.npts_total;
            one_per_pass = d.one_per_pass != 0;
        }
    }
    const int L = nlayers[b];
    if (L <= 0) return;   // sounding skipped by the caller (workgroup-uniform): none of its outputs are written
    if (L > Lmax) {       // bad row (would overrun the rows of sigma / thk and the LDS layer tables): flag it with NaNs, touch nothing else
        const double qnan = __builtin_nan("");
        if (pred != nullptr)
            for (int i = threadIdx.x; i < 2 * F; i += blockDim.x) pred[(size_t)b * 2 * F + i] = qnan;
        if (LIKE && threadIdx.x == 0) { chi2[b] = qnan; logL[b] = qnan; }
        return;
    }
    const gbp::MathCtx M = math_setup(sh_math);  // ends with __syncthreads()
    forward_body<LIKE, !SCALED>(M, sh_out, sh_dyn, chan, pts, npts_total, F, Lmax, L, sigma + (size_t)b * Lmax, thk + (size_t)b * Lmax,
                                height[b], LIKE ? obs + (size_t)b * 2 * F : nullptr, LIKE ? rel[b] : 0.0, LIKE ? add[b] : 0.0,
                                pred != nullptr ? pred + (size_t)b * 2 * F : nullptr, LIKE ? chi2 + b : nullptr, LIKE ? logL + b : nullptr,
                                sigma_direct, (int)(blockDim.x >> 6), (SCALED && row_scale != nullptr) ? row_scale[b] : 1.0, one_per_pass);
}

// k_fdem_forward<true> with the likelihood's model-independent terms prepared (gbp_gauss_prepare): `weight`[B, 2F] and `c0`[B] in
// place of rel / add, no per-row table set and no distance scale (the likelihood entries have neither).  ONE_WAVE is the launch with
// one wave per sounding (pick_waves from 8 192 soundings up): the workgroup size is a compile-time 64.
template <bool ONE_WAVE>
__global__ __launch_bounds__(ONE_WAVE ? 64 : 1024) void k_fdem_forward_prepared(const Channel* __restrict__ chan,
                                                                                const double* __restrict__ pts, int npts_total, int F,
                                                                                int Lmax, const int* __restrict__ nlayers,
                                                                                const double* __restrict__ sigma,
                                                                                const double* __restrict__ thk,
                                                                                const double* __restrict__ height,
                                                                                const double* __restrict__ obs,
                                                                                const double* __restrict__ weight,
                                                                                const double* __restrict__ c0, double* __restrict__ pred,
                                                                                double* __restrict__ chi2, double* __restrict__ logL,
                                                                                double sigma_direct, const BinDesc* __restrict__ bins,
                                                                                int bin0, int n_bins, const Channel* __restrict__ bin_chan,
                                                                                const double* __restrict__ bin_pts)
{
    __shared__ double sh_out[2 * GBP_MAX_FREQ];
    __shared__ MathLds sh_math;
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_dyn[];
    const int b = blockIdx.x;
    const int tid = ONE_WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x, nth = ONE_WAVE ? 64 : (int)blockDim.x;
    bool one_per_pass = false;
    if (bins != nullptr) {                                  // this sounding's abscissa window (see k_fdem_forward)
        const int slot = table_slot(height[b], 0, bin0, n_bins);
        if (slot >= 0) {
            const BinDesc d = bins[slot];
            chan = bin_chan + d.chan_off;
            pts = bin_pts + d.pts_off;
            npts_total = d.npts_total;
            one_per_pass = d.one_per_pass != 0;
        }
    }
    const int L = nlayers[b];
    if (L <= 0) return;   // as k_fdem_forward: a skipped sounding's outputs are not written, a bad row's are NaN
    if (L > Lmax) {
        const double qnan = __builtin_nan("");
        if (pred != nullptr)
            for (int i = tid; i < 2 * F; i += nth) pred[(size_t)b * 2 * F + i] = qnan;
        if (tid == 0) { chi2[b] = qnan; logL[b] = qnan; }
        return;
    }
    const gbp::MathCtx M = math_setup<true, ONE_WAVE>(sh_math);
    forward_body<true, true, true, ONE_WAVE>(M, sh_out, sh_dyn, chan, pts, npts_total, F, Lmax, L, sigma + (size_t)b * Lmax,
                                             thk + (size_t)b * Lmax, height[b], obs + (size_t)b * 2 * F, 0.0, 0.0,
                                             pred != nullptr ? pred + (size_t)b * 2 * F : nullptr, chi2 + b, logL + b, sigma_direct,
                                             ONE_WAVE ? 1 : (int)(blockDim.x >> 6), 1.0, one_per_pass, weight + (size_t)b * 2 * F, c0 + b);
}

// Jacobian (+ prediction) of ONE sounding by the first `nw_use` waves of the calling workgroup: the body of k_fdem_sens, also
// called by the persistent sampler kernel.  Each lane keeps d rTE / d ln sigma_m for its abscissa in LDS (row m, column
// lane, row stride 65 slots so that the row sums below are conflict-free), lane m then sums row m over the 64 abscissae.
// J[f, m] = Re(g * sum), J[F + f, m] = Im(g * sum).  Every thread of the workgroup must call it (one workgroup barrier).
//   sh_dyn: cplx D[nw_use][Lalloc][65] | LayerK lay[nw_use][Lalloc] | double t2[Lalloc]
#define GBP_SENS_STRIDE 65
template <bool EXACT, int NG>   // NG row groups of 8 layers are summed per evaluation: 1 / 2 / 4 for launches of <= 8 / 16 / more layers
__device__ __forceinline__ void sens_body(const gbp::MathCtx& M, unsigned char* sh_dyn, const Channel* __restrict__ chan,
                                          const double* __restrict__ pts, int npts_total, int F, int Lmax, int Lalloc, int L,
                                          const double* __restrict__ sig, const double* __restrict__ th, double alt,
                                          double* __restrict__ Jb /* [2F, Lmax] of this sounding */,
                                          double* __restrict__ pred_row /* [2F] or NULL */, int nw_use, int zero_to, double row_scale = 1.0,
                                          int share = 0, int n_shares = 1)
{   // share / n_shares: this workgroup evaluates the frequencies  wave * n_shares + share,  + nw_use * n_shares, ...  -- a frequency's
    // rows of J and pred depend on nothing but that frequency, so n_shares workgroups split a sounding's evaluation and write the same bits
    // zero_to: the unused columns L .. zero_to - 1 of every row are set to 0 (Lmax: the whole row, the public entries; the
    // sampler, whose consumers never read a column >= L, passes L rounded up to 8 and leaves the rest of the row alone)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = nw_use;
    cplx* sh_D = reinterpret_cast<cplx*>(sh_dyn) + (size_t)wave * Lalloc * GBP_SENS_STRIDE;
    gbp::LayerK* sh_lay = reinterpret_cast<gbp::LayerK*>(sh_dyn + (size_t)nwaves * Lalloc * GBP_SENS_STRIDE * sizeof(cplx)) +
                          (size_t)wave * Lalloc;
    double* sh_t2 = reinterpret_cast<double*>(sh_dyn + (size_t)nwaves * Lalloc * (GBP_SENS_STRIDE * sizeof(cplx) + sizeof(gbp::LayerK)));
    for (int k = threadIdx.x; k < L - 1; k += blockDim.x) sh_t2[k] = -2.0 * th[k];
    __syncthreads();
    if (wave >= nwaves) return;

    for (int f = wave * n_shares + share; f < F; f += nwaves * n_shares) {
        const Channel ch = chan[f];
        setup_layers(sh_lay, ch.wmu, sig, L, lane);
        const double hD = ch.hd0 - 2.0 * alt;
        // Row sums: lanes are arranged as 8 rows x 8 segments; lane (row, seg) adds the entries seg, seg + 8, ...
        // of row m0 + row (consecutive lanes -> consecutive 16-byte slots: conflict-free ds_read_b128), the 8
        // segment partials are combined with three xor-shuffles once per frequency.
        const int row = lane >> 3, seg = lane & 7;
        for (int m0 = 0; m0 < L; m0 += 8 * NG) {       // (runs once for L <= 8 NG; deeper models re-evaluate)
            double acc_re[NG], acc_im[NG];
            double fw_re = 0.0, fw_im = 0.0;       // this lane's share of the forward sum (fm_dlogc)
#pragma unroll
            for (int g = 0; g < NG; ++g) { acc_re[g] = 0.0; acc_im[g] = 0.0; }
            for (int j0 = 0; j0 < ch.npts; j0 += 64) {
                {
                    const int j = j0 + lane;
                    const bool valid = j < ch.npts;
                    gbp::Point pt = gbp::load_point(pts, npts_total, ch.off + (valid ? j : ch.npts - 1));
                    if (!valid) pt.coef = gbp::mk(0.0, 0.0);
                    if (row_scale != 1.0) gbp::scale_point(pt, row_scale);     // (wave-uniform, see forward_passes)
                    // (real exponents for every lane of the pass: exp only, same bits -- see gbp::hankel_term)
                    const cplx Q = __ballot(pt.ue.im != 0.0) == 0ull ? pt.coef * gbp::exp_neg(M, pt.ue.re * hD)
                                                                     : gbp::cexp_neg(M, pt.ue.re * hD, pt.ue.im * hD) * pt.coef;
                    const cplx t = gbp::sens_point<EXACT>(M, pt.a, L, sh_lay, sh_t2, pt.u0, Q, sh_D + lane,
                                                          GBP_SENS_STRIDE);
                    fw_re += t.re;
                    fw_im += t.im;
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (m0 + 8 * g < L) {              // wave-uniform
                        const int m = m0 + 8 * g + row;
                        if (m < L) {
                            const cplx* rowp = sh_D + (size_t)m * GBP_SENS_STRIDE + seg;
#pragma unroll
                            for (int i = 0; i < 8; ++i) { acc_re[g] += rowp[8 * i].re; acc_im[g] += rowp[8 * i].im; }
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            if (pred_row != nullptr && m0 == 0) {  // one wave owns the frequency: fixed summation order for any launch shape
                const double mine = wave_sum_pair(fw_re, fw_im, lane);   // lane 62: the real sum, lane 63: the imaginary one
                const double other = dpp_get<0xB1>(mine);
                if (lane == 62) pred_row[f] = ch.g_re * mine - ch.g_im * other;
                if (lane == 63) pred_row[F + f] = ch.g_re * mine + ch.g_im * other;
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (m0 + 8 * g < L) {
                    double sr = acc_re[g], si = acc_im[g];
                    sr += dpp_get<0xB1>(sr); si += dpp_get<0xB1>(si);       // the 8 segment partials of a row: lane ^ 1, ^ 2, then the
                    sr += dpp_get<0x4E>(sr); si += dpp_get<0x4E>(si);       // other quad of the 8 (row_half_mirror: every lane of a quad holds
                    sr += dpp_get<0x141>(sr); si += dpp_get<0x141>(si);     // the quad's sum by now) -- the sums of the xor shuffles, bit for bit
                    const int m = m0 + 8 * g + row;
                    if (m < L && seg == 0) {
                        Jb[(size_t)f * Lmax + m] = ch.g_re * sr - ch.g_im * si;
                        Jb[(size_t)(F + f) * Lmax + m] = ch.g_re * si + ch.g_im * sr;
                    }
                }
            }
        }
        for (int m = L + lane; m < zero_to; m += 64) {   // unused columns
            Jb[(size_t)f * Lmax + m] = 0.0;
            Jb[(size_t)(F + f) * Lmax + m] = 0.0;
        }
    }
}

template <bool EXACT, int NG>
__global__ __launch_bounds__(1024) void k_fdem_sens(const Channel* __restrict__ chan, const double* __restrict__ pts,
                                                    int npts_total, int F, int Lmax, int Lalloc,
                                                    const int* __restrict__ nlayers,
                                                    const double* __restrict__ sigma,
                                                    const double* __restrict__ thk,
                                                    const double* __restrict__ height, double* __restrict__ J,
                                                    double* __restrict__ pred, const BinDesc* __restrict__ bins, int bin0, int n_bins,
                                                    const Channel* __restrict__ bin_chan, const double* __restrict__ bin_pts,
                                                    int compact_rows, const int* __restrict__ row_set, const double* __restrict__ row_scale)
{
    __shared__ MathLds sh_math;
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_dyn[];
    const int b = blockIdx.x;
    const int L = nlayers[b];
    if (L <= 0) return;   // sounding skipped by the caller (workgroup-uniform)
    if (bins != nullptr) {                                  // this sounding's table set and abscissa window (see k_fdem_forward)
        const int slot = table_slot(height[b], row_set != nullptr ? row_set[b] : 0, bin0, n_bins);
        if (slot >= 0) {
            const BinDesc d = bins[slot];
            chan = bin_chan + d.chan_off;
            pts = bin_pts + d.pts_off;
            npts_total = d.npts_total;
        }
    }
    if (L > Lalloc || L > Lmax) {   // more layers than the launch was sized for: NaN row instead of an LDS / row overrun
        const double qnan = __builtin_nan("");
        const size_t n = (size_t)2 * F * Lmax;
        for (size_t i = threadIdx.x; i < n; i += blockDim.x) J[(size_t)b * n + i] = qnan;
        if (pred != nullptr)
            for (int i = threadIdx.x; i < 2 * F; i += blockDim.x) pred[(size_t)b * 2 * F + i] = qnan;
        return;
    }
    const gbp::MathCtx M = math_setup(sh_math);
    sens_body<EXACT, NG>(M, sh_dyn, chan, pts, npts_total, F, Lmax, Lalloc, L, sigma + (size_t)b * Lmax, thk + (size_t)b * Lmax,
                         height[b], J + (size_t)b * 2 * F * Lmax, pred != nullptr ? pred + (size_t)b * 2 * F : nullptr,
                         (int)(blockDim.x >> 6), compact_rows ? min(Lmax, (L + 7) & ~7) : Lmax, row_scale != nullptr ? row_scale[b] : 1.0);
}

// chi^2 / logL with an explicit per-channel standard deviation (TdemDataPoint.std is time dependent)
__global__ void k_gauss_loglike_std(int B, int N, const double* __restrict__ pred, const double* __restrict__ obs,
                                    const double* __restrict__ sd, double* __restrict__ chi2,
                                    double* __restrict__ logL)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;
    const double* p = pred + (size_t)b * N;
    const double* o = obs + (size_t)b * N;
    const double* s = sd + (size_t)b * N;
    double s2 = 0.0, logdet = 0.0, na = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double oi = o[i];
        if (oi > 0.0) {
            const double r = (p[i] - oi) * (1.0 / s[i]);
            s2 += r * r;
            logdet += 2.0 * log(s[i]);
            na += 1.0;
        }
    }
    s2 = wave_sum(s2);
    logdet = wave_sum(logdet);
    na = wave_sum(na);
    if (lane == 0) {
        chi2[b] = s2;
        logL[b] = -(0.5 * na) * 1.8378770664093453 - 0.5 * logdet - 0.5 * s2;
    }
}

__global__ void k_gauss_loglike(int B, int N, const double* __restrict__ pred, const double* __restrict__ obs,
                                const double* __restrict__ rel, const double* __restrict__ add,
                                double* __restrict__ chi2, double* __restrict__ logL)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;
    loglike_wave(N, pred + (size_t)b * N, obs + (size_t)b * N, rel[b], add[b], lane, chi2 + b, logL + b);
}

// The model-independent terms of loglike_wave, once per batch of data and error levels (gbp_gauss_prepare): per channel the factor
// 1 / sqrt(var) by loglike_wave's own expression (0 for an inactive channel, which loglike_wave_prepared never reads), per sounding
// c0 = -(0.5 na) ln 2pi - 0.5 logdet with na and logdet summed by loglike_wave's trees (wave_sum; lane 63 of wave_sum_pair).
__global__ void k_gauss_prepare(int B, int N, const double* __restrict__ obs, const double* __restrict__ rel,
                                const double* __restrict__ add, double* __restrict__ weight, double* __restrict__ c0)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;
    const double* o_row = obs + (size_t)b * N;
    double* w_row = weight + (size_t)b * N;
    const double rel_b = rel[b], add_b = add[b];
    double logdet = 0.0, na = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double o = o_row[i];
        const bool active = o > 0.0;
        const double ro = rel_b * o;
        const double var = ro * ro + add_b * add_b;
        double w = 0.0;
        if (active) {
            w = 1.0 / sqrt(var);
            logdet += log(var);
            na += 1.0;
        }
        w_row[i] = w;
    }
    const double mine = wave_sum_pair(0.0, logdet, lane);
    na = wave_sum(na);
    if (lane == 63) c0[b] = -(0.5 * na) * 1.8378770664093453 - 0.5 * mine;
}

// Per-sounding input / output status word (SURVEY 8b "Errors": validate, flag per sounding, never abort the batch).
__global__ void k_fdem_validate(int B, int Lmax, int N, const int* __restrict__ nlayers, const double* __restrict__ sigma,
                                const double* __restrict__ thk, const double* __restrict__ height,
                                const double* __restrict__ pred, int* __restrict__ status)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int st = 0;
    const int L = nlayers[b];
    if (L < 1 || L > Lmax) st |= GBP_ROW_BAD_NLAYERS;
    const int Lc = (L < 1 || L > Lmax) ? 0 : L;   // a row with a bad layer count has no meaningful layers to check
    for (int k = 0; k < Lc; ++k) {
        const double s = sigma[(size_t)b * Lmax + k];
        if (!(s > 0.0) || !(s < 1.7976931348623157e308)) st |= GBP_ROW_BAD_SIGMA;
        if (k < Lc - 1) {
            const double t = thk[(size_t)b * Lmax + k];
            if (!(t > 0.0) || !(t < 1.7976931348623157e308)) st |= GBP_ROW_BAD_THICKNESS;
        }
    }
    const double h = height[b];
    if (!(h >= 0.0) || !(h < 1.7976931348623157e308)) st |= GBP_ROW_BAD_HEIGHT;
    if (pred != nullptr)
        for (int i = 0; i < N; ++i) {
            const double v = pred[(size_t)b * N + i];
            if (!(v == v) || v > 1.7976931348623157e308 || v < -1.7976931348623157e308) st |= GBP_ROW_NONFINITE_OUTPUT;
        }
    status[b] = st;
}

// Evaluates the device math kernels element-wise (test hook: tests/test_gpu_math.py checks their
// accuracy on the real hardware, where v_rsq_f64 / v_rcp_f64 seeds differ from the host's).
__global__ void k_debug_math(int op, int n, const double* __restrict__ x, const double* __restrict__ y,
                             double* __restrict__ o0, double* __restrict__ o1)
{
    __shared__ MathLds sh_math;
    const gbp::MathCtx M = math_setup(sh_math);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double a = x[i], b = y ? y[i] : 0.0, r0 = 0.0, r1 = 0.0;
        switch (op) {
        case 0: r0 = gbp::exp_neg(M, a); break;
        case 1: gbp::sincos_tab(M, a, r0, r1); break;
        case 2: { cplx z = gbp::csqrt_upper(a, b); r0 = z.re; r1 = z.im; break; }
        case 3: r0 = gbp::rcp(a); break;
        case 4: r0 = gbp::rsq_seed(a); break;
        case 5: r0 = gbp::rcp_seed(a); break;
        case 6: gbp::sqrt_rsqrt(a, r0, r1); break;
        case 7: r0 = gbp::log_pos(a); break;
        case 8: gbp::sincos_quadrant(a, r0, r1); break;
        default: break;
        }
        o0[i] = r0;
        if (o1) o1[i] = r1;
    }
}

// ------------------------------------------------------------------------------------------
// host: system tables
// ------------------------------------------------------------------------------------------
namespace {

typedef std::complex<double> zc;

size_t dyn_lds_bytes(int nw, int Lmax, int passes)
{
    return (size_t)nw * 2 * Lmax * sizeof(gbp::LayerK) + (size_t)2 * passes * sizeof(cplx) + (size_t)Lmax * sizeof(double);
}

// waves per workgroup: enough workgroups x waves to fill 256 CUs x 8 waves even for small batches.  `waves` > 0 is the
// caller's explicit choice (the *_ex entries).  Results do not depend on it (forward_passes).
int pick_waves(int B, int F, int Lmax, int max_waves, int waves)
{
    // measured (scripts/sweep_waves.py, 10 frequencies x 8 layers, default abscissa windows = 10 passes per sounding): one wave
    // per sounding is best once every SIMD has a queue of soundings -- from 8 192 soundings (66.9 / 70.0 / 71.0 / 70.7 M evals/s at
    // 8 192 / 16 384 / 32 768 / 65 536 against 65.5 / 67.6 / 67.5 / 69.6 M with four waves, whose 10 passes split 3 3 2 2); below
    // that 4 waves per sounding balance the tail better (61.4 vs 60.9 M at 4 096, 56.7 vs 47.3 M at 2 048), and small batches need
    // 8192 / B waves to fill the chip at all.  (Round 2 switched at 49 152, measured with 19 passes per sounding.)
    const int heuristic = B >= 8192 ? 1 : std::max(4, (8192 + B - 1) / B);
    int nw = waves > 0 ? waves : heuristic;
    if (nw > max_waves) nw = max_waves;
    if (nw > 16) nw = 16;
    while (nw > 1 && dyn_lds_bytes(nw, Lmax, max_waves) > 60000) --nw;
    if (nw < 1) nw = 1;
    return nw;
}

const int GBP_MAX_LAYERS = 1024;  // LDS budget: (32 nw + 8) * Lmax bytes <= 64 KiB at nw = 1

gbp_status check_batch(const gbp_fdem_system* sys, int B, int Lmax, const void* a, const void* b, const void* c,
                       const void* d)
{
    if (!sys) return fail(GBP_ERR_INVALID_ARG, "system handle is NULL%s");
    if (B < 0 || Lmax < 1) return fail(GBP_ERR_INVALID_ARG, "B must be >= 0 and Lmax >= 1%s");
    if (Lmax > GBP_MAX_LAYERS) return fail(GBP_ERR_INVALID_ARG, "Lmax must be <= 1024%s");
    if (B > 0 && (!a || !b || !c || !d)) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    return GBP_OK;
}

// per-row table sets need the descriptors gbp_hankel_system_add_bins builds after the last gbp_hankel_system_add_set
gbp_status check_row_sets(const gbp_fdem_system* sys, const int32_t* set_of_row)
{
    if (set_of_row != nullptr && !sys->extra_sets.empty() && sys->d_bins == nullptr)
        return fail(GBP_ERR_INVALID_ARG, "table sets need their descriptors: call gbp_hankel_system_add_bins after the last add_set%s");
    return GBP_OK;
}

}  // namespace

static gbp_status fm_dlogc_launch(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers, const double* sigma,
                                  const double* thk, const double* height, double* pred, double* J, int max_layers, int exact,
                                  int waves, int compact_rows, const int32_t* set_of_row, void* stream, const double* row_scale = nullptr);

extern "C" {

const char* gbp_version(void) { return "geobipy_amd 0.2 (gfx950)"; }
const char* gbp_last_error(void) { return g_err; }

gbp_status gbp_device_count(int* count)
{
    if (!count) return fail(GBP_ERR_INVALID_ARG, "count is NULL%s");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(GBP_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return GBP_OK;
}

gbp_status gbp_fdem_system_create(int nF, const int32_t* tid, const double* frequencies, const double* tx_z,
                                  const double* rx_z, const double* tx_moment, const double* scale,
                                  const double* rx_off, const double* separation, const double* w0,
                                  const double* lamda0, const double* w1, const double* lamda1,
                                  gbp_fdem_system** out)
{
    return gbp_fdem_system_create_windowed(nF, tid, frequencies, tx_z, rx_z, tx_moment, scale, rx_off, separation, w0,
                                           lamda0, w1, lamda1, 0.0, 0.0, out);
}

gbp_status gbp_fdem_system_create_windowed(int nF, const int32_t* tid, const double* frequencies, const double* tx_z,
                                           const double* rx_z, const double* tx_moment, const double* scale,
                                           const double* rx_off, const double* separation, const double* w0,
                                           const double* lamda0, const double* w1, const double* lamda1,
                                           double eps_ppm, double min_altitude, gbp_fdem_system** out)
{
    if (!out) return fail(GBP_ERR_INVALID_ARG, "out is NULL%s");
    *out = nullptr;
    gbp_fdem_system* s = new (std::nothrow) gbp_fdem_system();
    if (!s) return fail(GBP_ERR_INVALID_ARG, "out of host memory%s");
    const char* msg = "";
    int rc = gbp::build_system_tables(nF, tid, frequencies, tx_z, rx_z, tx_moment, scale, rx_off, separation, w0,
                                      lamda0, w1, lamda1, &s->t, &msg);
    if (rc != GBP_OK) { delete s; return fail(rc, "%s", msg); }
    if (eps_ppm > 0.0 && !(min_altitude >= 0.0)) { delete s; return fail(GBP_ERR_INVALID_ARG, "min_altitude must be >= 0%s"); }
    gbp::window_system_tables(&s->t, eps_ppm, min_altitude);
    s->set_sigma_direct();
    const std::vector<double>& soa = s->t.soa;

    hipError_t e = hipMalloc((void**)&s->d_chan, sizeof(Channel) * nF);
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_pts, sizeof(double) * soa.size());
    if (e == hipSuccess) e = hipMemcpy(s->d_chan, s->t.chan.data(), sizeof(Channel) * nF, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_pts, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        gbp_fdem_system_destroy(s);
        return fail(GBP_ERR_HIP, "system table upload failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return GBP_OK;
}

gbp_status gbp_fdem_system_create_binned(int nF, const int32_t* tid, const double* frequencies, const double* tx_z,
                                         const double* rx_z, const double* tx_moment, const double* scale,
                                         const double* rx_off, const double* separation, const double* w0,
                                         const double* lamda0, const double* w1, const double* lamda1, double eps_ppm,
                                         int first_altitude_m, int n_bins, gbp_fdem_system** out)
{
    if (!out) return fail(GBP_ERR_INVALID_ARG, "out is NULL%s");
    *out = nullptr;
    if (!(eps_ppm > 0.0) || first_altitude_m < 0 || n_bins < 1 || n_bins > 1024)
        return fail(GBP_ERR_INVALID_ARG, "eps_ppm > 0, first_altitude_m >= 0 and 1 <= n_bins <= 1024 are required%s");
    gbp_fdem_system* s = nullptr;
    gbp_status st = gbp_fdem_system_create(nF, tid, frequencies, tx_z, rx_z, tx_moment, scale, rx_off, separation, w0, lamda0, w1, lamda1, &s);
    if (st != GBP_OK) return st;
    st = gbp_hankel_system_add_bins(s, eps_ppm, 0, first_altitude_m, n_bins);
    if (st != GBP_OK) {
        gbp_fdem_system_destroy(s);
        return st;
    }
    *out = s;
    return GBP_OK;
}

static void drop_device_bins(gbp_fdem_system* s)
{
    if (s->d_bins) { (void)hipFree(s->d_bins); s->d_bins = nullptr; }
    if (s->d_bin_chan) { (void)hipFree(s->d_bin_chan); s->d_bin_chan = nullptr; }
    if (s->d_bin_pts) { (void)hipFree(s->d_bin_pts); s->d_bin_pts = nullptr; }
    s->n_bins = 0;
    s->bin_npts.clear();
}

gbp_status gbp_hankel_system_clear_bins(gbp_fdem_system* s)
{
    if (!s) return fail(GBP_ERR_INVALID_ARG, "system handle is NULL%s");
    drop_device_bins(s);
    s->packs.clear();
    s->pack_eps = -1.0;
    return GBP_OK;
}

gbp_status gbp_hankel_system_add_bins(gbp_fdem_system* s, double eps, int relative, int first_altitude_m, int n_bins)
{
    if (!s) return fail(GBP_ERR_INVALID_ARG, "system handle is NULL%s");
    const bool sets_only = n_bins == 0 && eps == 0.0 && !s->extra_sets.empty();     // descriptors of the further sets' full tables
    if (!sets_only && (!(eps > 0.0) || first_altitude_m < 0 || n_bins < 1 || n_bins > 1024))
        return fail(GBP_ERR_INVALID_ARG, "eps > 0, first_altitude_m >= 0 and 1 <= n_bins <= 1024 are required%s");
    drop_device_bins(s);                                                        // (replaces an earlier set)
    if (s->pack_eps != eps || s->pack_relative != (relative != 0) || s->pack_first != first_altitude_m || s->pack_bins != n_bins) {
        s->packs.clear();
        s->pack_eps = eps; s->pack_relative = relative != 0; s->pack_first = first_altitude_m; s->pack_bins = n_bins;
    }
    try {
        for (int k = (int)s->packs.size(); k <= (int)s->extra_sets.size(); ++k) {   // only the sets that are new since the last call
            const gbp::SystemTables& full = k == 0 ? s->t : s->extra_sets[k - 1];
            gbp_fdem_system::Pack pk;
            auto push = [&](const gbp::SystemTables& t) {
                BinDesc d;
                d.chan_off = (int)pk.chans.size();
                d.npts_total = t.npts;
                d.pts_off = (long long)pk.pts.size();
                d.one_per_pass = t.npts == 64 * (int)t.chan.size();
                for (size_t f = 0; f < t.chan.size(); ++f) d.one_per_pass &= t.chan[f].off == 64 * (int)f && t.chan[f].npts == 64;
                d.spare = 0;
                pk.desc.push_back(d);
                pk.chans.insert(pk.chans.end(), t.chan.begin(), t.chan.end());
                pk.pts.insert(pk.pts.end(), t.soa.begin(), t.soa.end());
            };
            if (k > 0) push(full);                           // a further set's own tables (soundings below the first bin)
            for (int i = 0; i < n_bins; ++i) {
                gbp::SystemTables t = full;                  // the exact tables, then windowed for altitude >= first + i metres
                gbp::window_system_tables(&t, eps, (double)(first_altitude_m + i), relative != 0);
                push(t);
            }
            s->packs.push_back(std::move(pk));
        }
    } catch (const std::bad_alloc&) {
        s->packs.clear();
        s->pack_eps = -1.0;
        return fail(GBP_ERR_INVALID_ARG, "out of host memory for the abscissa windows of the table sets%s");
    }
    std::vector<BinDesc> desc;
    size_t n_chan = 0, n_pts = 0;
    for (const auto& pk : s->packs) {
        for (BinDesc d : pk.desc) { d.chan_off += (int)n_chan; d.pts_off += (long long)n_pts; desc.push_back(d); }
        n_chan += pk.chans.size();
        n_pts += pk.pts.size();
    }
    s->bin_npts.resize(n_bins);
    for (int i = 0; i < n_bins; ++i) s->bin_npts[i] = s->packs[0].desc[i].npts_total;
    s->bin0 = first_altitude_m;
    hipError_t e = hipMalloc((void**)&s->d_bins, sizeof(BinDesc) * std::max<size_t>(desc.size(), 1));
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_bin_chan, sizeof(Channel) * std::max<size_t>(n_chan, 1));
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_bin_pts, sizeof(double) * std::max<size_t>(n_pts, 1));
    if (e == hipSuccess && !desc.empty()) e = hipMemcpy(s->d_bins, desc.data(), sizeof(BinDesc) * desc.size(), hipMemcpyHostToDevice);
    n_chan = n_pts = 0;
    for (const auto& pk : s->packs) {
        if (e == hipSuccess && !pk.chans.empty())
            e = hipMemcpy(s->d_bin_chan + n_chan, pk.chans.data(), sizeof(Channel) * pk.chans.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !pk.pts.empty())
            e = hipMemcpy(s->d_bin_pts + n_pts, pk.pts.data(), sizeof(double) * pk.pts.size(), hipMemcpyHostToDevice);
        n_chan += pk.chans.size();
        n_pts += pk.pts.size();
    }
    if (e != hipSuccess) {
        drop_device_bins(s);
        return fail(GBP_ERR_HIP, "bin table upload failed: %s", hipGetErrorString(e));
    }
    s->n_bins = n_bins;
    return GBP_OK;
}

gbp_status gbp_hankel_system_add_set(gbp_fdem_system* s, const double* hd0, const double* tables)
{
    if (!s || !hd0 || !tables) return fail(GBP_ERR_INVALID_ARG, "NULL argument%s");
    gbp::SystemTables t = s->t;                          // same frequencies, weights and point counts: other altitude terms and points
    for (int f = 0; f < t.nF; ++f) t.chan[f].hd0 = hd0[f];
    t.soa.assign(tables, tables + (size_t)GBP_PT_FIELDS * t.npts);
    s->extra_sets.push_back(std::move(t));
    drop_device_bins(s);                                 // descriptors are rebuilt by the next gbp_hankel_system_add_bins (the
                                                         // windows of the sets that were there are kept on the host)
    return GBP_OK;
}

gbp_status gbp_fdem_system_bin_points(const gbp_fdem_system* sys, int altitude_m, int* npts)
{
    if (!sys || !npts) return fail(GBP_ERR_INVALID_ARG, "NULL argument%s");
    if (sys->n_bins == 0 || altitude_m < sys->bin0) { *npts = sys->t.npts; return GBP_OK; }
    *npts = sys->bin_npts[std::min(altitude_m - sys->bin0, sys->n_bins - 1)];
    return GBP_OK;
}

gbp_status gbp_hankel_system_create_raw(int nF, const int32_t* npts, const double* wmu, const double* hd0,
                                        const double* g, const double* tables, gbp_fdem_system** out)
{
    if (!out) return fail(GBP_ERR_INVALID_ARG, "out is NULL%s");
    *out = nullptr;
    if (nF < 1 || nF > GBP_MAX_FREQ) return fail(GBP_ERR_INVALID_ARG, "nF must be in [1, 128]%s");
    if (!npts || !wmu || !hd0 || !g || !tables) return fail(GBP_ERR_INVALID_ARG, "NULL system array%s");
    gbp_fdem_system* s = new (std::nothrow) gbp_fdem_system();
    if (!s) return fail(GBP_ERR_INVALID_ARG, "out of host memory%s");
    gbp::SystemTables& t = s->t;
    t.nF = nF;
    t.chan.assign(nF, Channel());
    t.h0.assign(2 * (size_t)nF, 1.0);
    int P = 0;
    for (int f = 0; f < nF; ++f) {
        if (npts[f] < 64 || !(wmu[f] > 0.0) || !std::isfinite(wmu[f])) {
            delete s;
            return fail(GBP_ERR_BAD_SYSTEM, "each frequency needs >= 64 points and wmu > 0%s");
        }
        Channel& ch = t.chan[f];
        ch.wmu = wmu[f]; ch.w2me = 0.0; ch.hd0 = hd0[f]; ch.g_re = g[2 * f]; ch.g_im = g[2 * f + 1];
        ch.off = P; ch.npts = npts[f]; ch.real_exp = 0; ch.tid = 0;
        if (npts[f] > t.max_pts) t.max_pts = npts[f];
        P += npts[f];
    }
    t.npts = P;
    t.soa.assign(tables, tables + (size_t)GBP_PT_FIELDS * P);
    s->set_sigma_direct();
    const std::vector<double>& soa = t.soa;
    hipError_t e = hipMalloc((void**)&s->d_chan, sizeof(Channel) * nF);
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_pts, sizeof(double) * soa.size());
    if (e == hipSuccess) e = hipMemcpy(s->d_chan, s->t.chan.data(), sizeof(Channel) * nF, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_pts, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        gbp_fdem_system_destroy(s);
        return fail(GBP_ERR_HIP, "system table upload failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return GBP_OK;
}

void gbp_fdem_system_destroy(gbp_fdem_system* sys)
{
    if (!sys) return;
    if (sys->d_chan) (void)hipFree(sys->d_chan);
    if (sys->d_pts) (void)hipFree(sys->d_pts);
    if (sys->d_bins) (void)hipFree(sys->d_bins);
    if (sys->d_bin_chan) (void)hipFree(sys->d_bin_chan);
    if (sys->d_bin_pts) (void)hipFree(sys->d_bin_pts);
    delete sys;
}

gbp_status gbp_fdem_system_npoints(const gbp_fdem_system* sys, int* npts)
{
    if (!sys || !npts) return fail(GBP_ERR_INVALID_ARG, "NULL argument%s");
    *npts = sys->t.npts;
    return GBP_OK;
}

gbp_status gbp_fdem_system_nfreq(const gbp_fdem_system* sys, int* nF)
{
    if (!sys || !nF) return fail(GBP_ERR_INVALID_ARG, "NULL argument%s");
    *nF = sys->t.nF;
    return GBP_OK;
}

gbp_status gbp_fdem_system_h0(const gbp_fdem_system* sys, double* out)
{
    if (!sys || !out) return fail(GBP_ERR_INVALID_ARG, "NULL argument%s");
    std::memcpy(out, sys->t.h0.data(), sizeof(double) * sys->t.h0.size());
    return GBP_OK;
}

gbp_status gbp_fdem_forward(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                            const double* sigma, const double* thk, const double* height, double* pred,
                            void* stream)
{
    return gbp_fdem_forward_ex(sys, B, Lmax, nlayers, sigma, thk, height, pred, 0, stream);
}

gbp_status gbp_fdem_forward_ex(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                               const double* sigma, const double* thk, const double* height, double* pred,
                               int waves, void* stream)
{
    return gbp_fdem_forward_rows_ex(sys, B, Lmax, nlayers, sigma, thk, height, pred, nullptr, waves, stream);
}

gbp_status gbp_fdem_forward_rows_ex(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                    const double* sigma, const double* thk, const double* height, double* pred,
                                    const int32_t* set_of_row, int waves, void* stream)
{
    return gbp_fdem_forward_rows_scaled(sys, B, Lmax, nlayers, sigma, thk, height, pred, set_of_row, nullptr, waves, stream);
}

gbp_status gbp_fdem_forward_rows_scaled(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                        const double* sigma, const double* thk, const double* height, double* pred,
                                        const int32_t* set_of_row, const double* row_scale, int waves, void* stream)
{
    gbp_status st = check_batch(sys, B, Lmax, nlayers, sigma, thk, height);
    if (st != GBP_OK) return st;
    if (waves < 0 || waves > 16) return fail(GBP_ERR_INVALID_ARG, "waves must be in [0, 16]%s");
    if (B == 0) return GBP_OK;
    if (!pred) return fail(GBP_ERR_INVALID_ARG, "pred is NULL%s");
    if ((st = check_row_sets(sys, set_of_row)) != GBP_OK) return st;
    const int nw = pick_waves(B, sys->t.nF, Lmax, (sys->t.npts + 63) / 64, waves);
    auto kernel = row_scale != nullptr ? k_fdem_forward<false, true> : k_fdem_forward<false, false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(64 * nw), dyn_lds_bytes(nw, Lmax, (sys->t.npts + 63) / 64), (hipStream_t)stream, sys->d_chan,
                       sys->d_pts, sys->t.npts, sys->t.nF, Lmax, nlayers, sigma, thk, height, nullptr, nullptr,
                       nullptr, pred, nullptr, nullptr, sys->sigma_direct, sys->d_bins, sys->bin0, sys->n_bins, sys->d_bin_chan, sys->d_bin_pts,
                       set_of_row, row_scale);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

gbp_status gbp_gauss_loglike(int B, int N, const double* pred, const double* obs, const double* rel,
                             const double* add, double* chi2, double* logL, void* stream)
{
    if (B < 0 || N < 1) return fail(GBP_ERR_INVALID_ARG, "B must be >= 0 and N >= 1%s");
    if (B == 0) return GBP_OK;
    if (!pred || !obs || !rel || !add || !chi2 || !logL) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    const int wpb = 4;
    hipLaunchKernelGGL(k_gauss_loglike, dim3((B + wpb - 1) / wpb), dim3(64 * wpb), 0, (hipStream_t)stream, B, N,
                       pred, obs, rel, add, chi2, logL);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

gbp_status gbp_gauss_loglike_std(int B, int N, const double* pred, const double* obs, const double* sd, double* chi2,
                                 double* logL, void* stream)
{
    if (B < 0 || N < 1) return fail(GBP_ERR_INVALID_ARG, "B must be >= 0 and N >= 1%s");
    if (B == 0) return GBP_OK;
    if (!pred || !obs || !sd || !chi2 || !logL) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    const int wpb = 4;
    hipLaunchKernelGGL(k_gauss_loglike_std, dim3((B + wpb - 1) / wpb), dim3(64 * wpb), 0, (hipStream_t)stream, B, N,
                       pred, obs, sd, chi2, logL);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

gbp_status gbp_fdem_forward_loglike(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                    const double* sigma, const double* thk, const double* height,
                                    const double* obs, const double* rel, const double* add, double* pred,
                                    double* chi2, double* logL, void* stream)
{
    return gbp_fdem_forward_loglike_ex(sys, B, Lmax, nlayers, sigma, thk, height, obs, rel, add, pred, chi2, logL, 0, stream);
}

gbp_status gbp_fdem_forward_loglike_ex(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                       const double* sigma, const double* thk, const double* height,
                                       const double* obs, const double* rel, const double* add, double* pred,
                                       double* chi2, double* logL, int waves, void* stream)
{
    gbp_status st = check_batch(sys, B, Lmax, nlayers, sigma, thk, height);
    if (st != GBP_OK) return st;
    if (waves < 0 || waves > 16) return fail(GBP_ERR_INVALID_ARG, "waves must be in [0, 16]%s");
    if (B == 0) return GBP_OK;
    if (!obs || !rel || !add || !chi2 || !logL) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    const int nw = pick_waves(B, sys->t.nF, Lmax, (sys->t.npts + 63) / 64, waves);
    hipLaunchKernelGGL(k_fdem_forward<true>, dim3(B), dim3(64 * nw), dyn_lds_bytes(nw, Lmax, (sys->t.npts + 63) / 64), (hipStream_t)stream, sys->d_chan,
                       sys->d_pts, sys->t.npts, sys->t.nF, Lmax, nlayers, sigma, thk, height, obs, rel, add, pred,
                       chi2, logL, sys->sigma_direct, sys->d_bins, sys->bin0, sys->n_bins, sys->d_bin_chan, sys->d_bin_pts, nullptr, nullptr);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

gbp_status gbp_gauss_prepare(int B, int N, const double* obs, const double* rel, const double* add, double* weight, double* c0,
                             void* stream)
{
    if (B < 0 || N < 1) return fail(GBP_ERR_INVALID_ARG, "B must be >= 0 and N >= 1%s");
    if (B == 0) return GBP_OK;
    if (!obs || !rel || !add || !weight || !c0) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    const int wpb = 4;
    hipLaunchKernelGGL(k_gauss_prepare, dim3((B + wpb - 1) / wpb), dim3(64 * wpb), 0, (hipStream_t)stream, B, N, obs, rel, add,
                       weight, c0);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

gbp_status gbp_fdem_forward_loglike_prepared(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                             const double* sigma, const double* thk, const double* height,
                                             const double* obs, const double* weight, const double* c0, double* pred,
                                             double* chi2, double* logL, void* stream)
{
    return gbp_fdem_forward_loglike_prepared_ex(sys, B, Lmax, nlayers, sigma, thk, height, obs, weight, c0, pred, chi2, logL, 0, stream);
}

gbp_status gbp_fdem_forward_loglike_prepared_ex(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                                const double* sigma, const double* thk, const double* height,
                                                const double* obs, const double* weight, const double* c0, double* pred,
                                                double* chi2, double* logL, int waves, void* stream)
{
    gbp_status st = check_batch(sys, B, Lmax, nlayers, sigma, thk, height);
    if (st != GBP_OK) return st;
    if (waves < 0 || waves > 16) return fail(GBP_ERR_INVALID_ARG, "waves must be in [0, 16]%s");
    if (B == 0) return GBP_OK;
    if (!obs || !weight || !c0 || !chi2 || !logL) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    const int passes = (sys->t.npts + 63) / 64;
    const int nw = pick_waves(B, sys->t.nF, Lmax, passes, waves);
    auto kernel = nw == 1 ? k_fdem_forward_prepared<true> : k_fdem_forward_prepared<false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(64 * nw), dyn_lds_bytes(nw, Lmax, passes), (hipStream_t)stream, sys->d_chan, sys->d_pts,
                       sys->t.npts, sys->t.nF, Lmax, nlayers, sigma, thk, height, obs, weight, c0, pred, chi2, logL, sys->sigma_direct,
                       sys->d_bins, sys->bin0, sys->n_bins, sys->d_bin_chan, sys->d_bin_pts);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

gbp_status gbp_fdem_validate(int B, int Lmax, int N, const int32_t* nlayers, const double* sigma, const double* thk,
                             const double* height, const double* pred, int32_t* status, void* stream)
{
    if (B < 0 || Lmax < 1 || N < 0) return fail(GBP_ERR_INVALID_ARG, "B must be >= 0, Lmax >= 1, N >= 0%s");
    if (B == 0) return GBP_OK;
    if (!nlayers || !sigma || !thk || !height || !status) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    hipLaunchKernelGGL(k_fdem_validate, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, Lmax, N, nlayers, sigma,
                       thk, height, pred, status);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// average time of `reps` launches of `launch` on `stream`, by two events around them
extern "C++" template <class Launch>
static gbp_status time_launches(void* stream, int reps, float* avg_ms, Launch launch)
{
    if (!avg_ms || reps < 1) return fail(GBP_ERR_INVALID_ARG, "avg_ms NULL or reps < 1%s");
    hipEvent_t e0, e1;
    GBP_HIP(hipEventCreate(&e0));
    GBP_HIP(hipEventCreate(&e1));
    gbp_status st = GBP_OK;
    float ms = 0.f;
    hipError_t e = hipEventRecord(e0, (hipStream_t)stream);
    for (int i = 0; i < reps && st == GBP_OK && e == hipSuccess; ++i) st = launch();
    if (e == hipSuccess) e = hipEventRecord(e1, (hipStream_t)stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(GBP_ERR_HIP, "timing events: %s", hipGetErrorString(e));
    *avg_ms = ms / reps;
    return st;
}

gbp_status gbp_bench_time_forward_loglike(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                         const double* sigma, const double* thk, const double* height,
                                         const double* obs, const double* rel, const double* add, double* pred,
                                         double* chi2, double* logL, void* stream, int reps, float* avg_ms)
{
    return time_launches(stream, reps, avg_ms, [&] {
        return gbp_fdem_forward_loglike(sys, B, Lmax, nlayers, sigma, thk, height, obs, rel, add, pred, chi2, logL, stream);
    });
}

gbp_status gbp_bench_time_forward_loglike_prepared(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                                  const double* sigma, const double* thk, const double* height,
                                                  const double* obs, const double* weight, const double* c0, double* pred,
                                                  double* chi2, double* logL, void* stream, int reps, float* avg_ms)
{
    return time_launches(stream, reps, avg_ms, [&] {
        return gbp_fdem_forward_loglike_prepared(sys, B, Lmax, nlayers, sigma, thk, height, obs, weight, c0, pred, chi2, logL, stream);
    });
}

gbp_status gbp_debug_math(int op, int n, const double* x, const double* y, double* out0, double* out1, void* stream)
{
    if (n < 0 || op < 0 || op > 8) return fail(GBP_ERR_INVALID_ARG, "bad op or n%s");
    if (n == 0) return GBP_OK;
    if (!x || !out0) return fail(GBP_ERR_INVALID_ARG, "NULL device pointer%s");
    hipLaunchKernelGGL(k_debug_math, dim3(1024), dim3(256), 0, (hipStream_t)stream, op, n, x, y, out0, out1);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

gbp_status gbp_fdem_sensitivity(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                const double* sigma, const double* thk, const double* height, double* J,
                                void* stream)
{
    return gbp_fdem_sensitivity_ex(sys, B, Lmax, nlayers, sigma, thk, height, J, Lmax, 0, stream);
}

gbp_status gbp_fdem_sensitivity_ex(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers,
                                   const double* sigma, const double* thk, const double* height, double* J,
                                   int max_layers, int exact, void* stream)
{
    return gbp_fdem_fm_dlogc(sys, B, Lmax, nlayers, sigma, thk, height, nullptr, J, max_layers, exact, stream);
}

gbp_status gbp_fdem_fm_dlogc(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers, const double* sigma,
                             const double* thk, const double* height, double* pred, double* J, int max_layers, int exact,
                             void* stream)
{
    return gbp_fdem_fm_dlogc_ex(sys, B, Lmax, nlayers, sigma, thk, height, pred, J, max_layers, exact, 0, stream);
}

gbp_status gbp_fdem_fm_dlogc_ex(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers, const double* sigma,
                                const double* thk, const double* height, double* pred, double* J, int max_layers, int exact,
                                int waves, void* stream)
{
    return fm_dlogc_launch(sys, B, Lmax, nlayers, sigma, thk, height, pred, J, max_layers, exact, waves, 0, nullptr, stream);
}

gbp_status gbp_fdem_fm_dlogc_rows_ex(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers, const double* sigma,
                                     const double* thk, const double* height, double* pred, double* J, int max_layers, int exact,
                                     const int32_t* set_of_row, int waves, void* stream)
{
    return fm_dlogc_launch(sys, B, Lmax, nlayers, sigma, thk, height, pred, J, max_layers, exact, waves, 0, set_of_row, stream);
}

gbp_status gbp_fdem_fm_dlogc_rows_scaled(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers, const double* sigma,
                                         const double* thk, const double* height, double* pred, double* J, int max_layers, int exact,
                                         const int32_t* set_of_row, const double* row_scale, int waves, void* stream)
{
    return fm_dlogc_launch(sys, B, Lmax, nlayers, sigma, thk, height, pred, J, max_layers, exact, waves, 0, set_of_row, stream, row_scale);
}

}  // extern "C"

// compact_rows != 0 (the sampler's launches): only the columns up to the layer count rounded up to 8 are written
static gbp_status fm_dlogc_launch(const gbp_fdem_system* sys, int B, int Lmax, const int32_t* nlayers, const double* sigma,
                                  const double* thk, const double* height, double* pred, double* J, int max_layers, int exact,
                                  int waves, int compact_rows, const int32_t* set_of_row, void* stream, const double* row_scale)
{
    gbp_status st = check_batch(sys, B, Lmax, nlayers, sigma, thk, height);
    if (st != GBP_OK) return st;
    if (B == 0) return GBP_OK;
    if (!J) return fail(GBP_ERR_INVALID_ARG, "J is NULL%s");
    if ((st = check_row_sets(sys, set_of_row)) != GBP_OK) return st;
    if (max_layers < 1 || max_layers > Lmax) max_layers = Lmax;
    const size_t per_wave = (size_t)max_layers * (GBP_SENS_STRIDE * sizeof(cplx) + sizeof(gbp::LayerK));
    if (per_wave + (size_t)max_layers * 8 > 150000)
        return fail(GBP_ERR_INVALID_ARG, "too many layers for the Jacobian kernel's LDS working set (max ~140)%s");
    // one frequency per wave at a time, so the result does not depend on nw and nw should divide nF; `waves` is a
    // performance hint only (the sampler's launches, where only a fraction of the workgroups has work)
    if (waves < 0 || waves > 16) return fail(GBP_ERR_INVALID_ARG, "waves must be in [0, 16]%s");
    int nw = pick_waves(B, sys->t.nF, Lmax, sys->t.nF, waves);
    if (nw > sys->t.nF) nw = sys->t.nF;
    // LDS per workgroup: 60 KB keeps two workgroups per CU resident; small launches -- where a workgroup per CU is all there is, and a
    // deep model on one wave is a long tail (22 frequencies x 30 layers in sequence) -- may take most of a CU's 160 KB
    const size_t lds_cap = B <= 4096 ? 150000 : 60000;
    while (nw > 1 && nw * per_wave + (size_t)max_layers * 8 > lds_cap) --nw;
    const size_t lds = nw * per_wave + (size_t)max_layers * 8;
    auto launch = [&](auto kernel) -> gbp_status {
        if (lds > 48 * 1024) GBP_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3(B), dim3(64 * nw), lds, (hipStream_t)stream, sys->d_chan, sys->d_pts, sys->t.npts, sys->t.nF,
                           Lmax, max_layers, nlayers, sigma, thk, height, J, pred, sys->d_bins, sys->bin0, sys->n_bins, sys->d_bin_chan,
                           sys->d_bin_pts, compact_rows, set_of_row, row_scale);
        return GBP_OK;
    };
    // launches capped at 8 (the sampler's common case) / 16 layers use variants with one / two row groups: fewer VGPRs.  Deeper launches
    // sum FOUR row groups (32 layers) per evaluation -- 121 / 119 VGPRs, no scratch; the eight-group variant of rounds 1 - 5 spilled 11 - 13
    // registers (48 - 56 B per lane) under the 128-VGPR budget -- and a model of 33 or more layers takes a second evaluation (sens_body's m0
    // loop): the rows are the same sums in the same order, the same bits (tests/test_gpu_parity.py: the 30-layer fixtures)
    const int ng = max_layers <= 8 ? 1 : (max_layers <= 16 ? 2 : 4);
    if (exact) st = ng == 1 ? launch(k_fdem_sens<true, 1>) : (ng == 2 ? launch(k_fdem_sens<true, 2>) : launch(k_fdem_sens<true, 4>));
    else st = ng == 1 ? launch(k_fdem_sens<false, 1>) : (ng == 2 ? launch(k_fdem_sens<false, 2>) : launch(k_fdem_sens<false, 4>));
    if (st != GBP_OK) return st;
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

#include "gbp_rjmcmc.h"
#include "gbp_tdem.h"
#include "gbp_hostpack.h"
#include "gbp_hitmap.h"
#include "gbp_ensemble.h"
#include "gbp_ensemble_diag.h"

// Per-depth mean and 5 / 50 / 95 % points of log10 conductivity of B hit maps [B, nv, nz] (depth fastest) -> four [B, nz] arrays
extern "C" gbp_status gbp_hitmap_statistics(int B, int nv, int nz, const int32_t* hitmap, const double* log_mean_prior, double half_width,
                                            double* mean, double* p05, double* p50, double* p95, void* stream)
{
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (B < 0 || nv < 1 || nz < 1 || !hitmap || !log_mean_prior || !mean || !p05 || !p50 || !p95)
        return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_statistics: NULL pointer or non-positive size%s");
    hipLaunchKernelGGL(hitmap::k_hitmap_stats, dim3(B, (nz + 255) / 256), dim3(256), 0, (hipStream_t)stream, nv, nz, hitmap, log_mean_prior, half_width,
                       mean, p05, p50, p95);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// Per-column moments of B hit maps [B, nv, nz] for the line products: mean (as gbp_hitmap_statistics), mode index, n_q quantile indices
// (q: host array, 0 < q < 1, n_q <= 8), total and sum c ln c -> [B, nz] arrays ([n_q, B, nz] for q_idx).  T: the maps' count type.
template <typename T>
static gbp_status hitmap_products(int B, int nv, int nz, const T* hitmap, const double* log_mean_prior, double half_width, int n_q,
                                  const double* q, double* mean, int32_t* mode_idx, int32_t* q_idx, int64_t* total, double* s1, void* stream)
{
    if (B < 0 || nv < 1 || nz < 1 || n_q < 0 || n_q > 8 || (n_q > 0 && !q))
        return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_products: non-positive size, n_q outside 0 .. 8 or q NULL%s");
    hitmap::Quantiles qs = {};
    qs.n = n_q;
    for (int k = 0; k < n_q; ++k) {
        if (!(q[k] > 0.0 && q[k] < 1.0)) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_products: every quantile must lie in (0, 1)%s");
        qs.q[k] = q[k];
    }
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!hitmap || !log_mean_prior || !mean || !mode_idx || (n_q > 0 && !q_idx) || !total || !s1)
        return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_products: NULL pointer%s");
    if ((int64_t)B * nz > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_products: B * n_depth out of range%s");
    static_assert(sizeof(long long) == sizeof(int64_t), "int64_t is long long here");
    hipLaunchKernelGGL(hitmap::k_hitmap_products<T>, dim3(B, (nz + 255) / 256), dim3(256), 0, (hipStream_t)stream, nv, nz, hitmap, log_mean_prior,
                       half_width, qs, mean, mode_idx, q_idx, (long long*)total, s1);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

extern "C" gbp_status gbp_hitmap_products(int B, int nv, int nz, const int32_t* hitmap, const double* log_mean_prior, double half_width,
                                          int n_q, const double* q, double* mean, int32_t* mode_idx, int32_t* q_idx, int64_t* total,
                                          double* s1, void* stream)
{
    return hitmap_products<int>(B, nv, nz, hitmap, log_mean_prior, half_width, n_q, q, mean, mode_idx, q_idx, total, s1, stream);
}

// The same over int64 maps [B, nv, nz] (interval marginals: gbp_hitmap_intervals)
extern "C" gbp_status gbp_hitmap_products_i64(int B, int nv, int nz, const int64_t* hitmap, const double* log_mean_prior, double half_width,
                                              int n_q, const double* q, double* mean, int32_t* mode_idx, int32_t* q_idx, int64_t* total,
                                              double* s1, void* stream)
{
    return hitmap_products<long long>(B, nv, nz, (const long long*)hitmap, log_mean_prior, half_width, n_q, q, mean, mode_idx, q_idx, total, s1,
                                      stream);
}

// Class probabilities of B hit maps [B, nv, nz] for K classes in log10 conductivity (means / scales: host arrays of K values, scale the
// standard deviation) -> prob [B, K, nz], best [B, nz] (the most probable class) and best_p [B, nz] (its probability)
template <typename T>
static gbp_status hitmap_classes(int B, int nv, int nz, const T* hitmap, const double* log_mean_prior, double half_width, int K,
                                 const double* means, const double* scales, double* prob, int32_t* best, double* best_p, void* stream)
{
    if (B < 0 || nv < 1 || nz < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: negative or zero size%s");
    if (K < 1 || K > hitmap::MAX_CLASSES) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: K outside 1 .. 16%s");
    if (!means || !scales) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: means / scales NULL%s");
    hitmap::Classes cl = {};
    cl.n = K;
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(means[k])) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: every class mean must be finite%s");
        if (!(std::isfinite(scales[k]) && scales[k] > 0.0))
            return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: every class scale must be finite and positive%s");
        cl.mean[k] = means[k];
        cl.scale[k] = scales[k];
    }
    const int64_t lds = (int64_t)K * nv * (int64_t)sizeof(double);
    if (lds > 65536) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: the class table (K * n_value * 8 B) exceeds 64 KiB of LDS%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!hitmap || !log_mean_prior || !prob || !best || !best_p) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: NULL pointer%s");
    if ((int64_t)B * nz > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_classes: B * n_depth out of range%s");
    const dim3 grid(B, (nz + 255) / 256);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), (size_t)lds, (hipStream_t)stream, nv, nz, hitmap, log_mean_prior, half_width, cl, prob, best,
                           best_p);
    };
    if (K <= 1) launch(hitmap::k_hitmap_classes<1, T>);
    else if (K <= 2) launch(hitmap::k_hitmap_classes<2, T>);
    else if (K <= 4) launch(hitmap::k_hitmap_classes<4, T>);
    else if (K <= 8) launch(hitmap::k_hitmap_classes<8, T>);
    else launch(hitmap::k_hitmap_classes<16, T>);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

extern "C" gbp_status gbp_hitmap_classes(int B, int nv, int nz, const int32_t* hitmap, const double* log_mean_prior, double half_width, int K,
                                         const double* means, const double* scales, double* prob, int32_t* best, double* best_p, void* stream)
{
    return hitmap_classes<int>(B, nv, nz, hitmap, log_mean_prior, half_width, K, means, scales, prob, best, best_p, stream);
}

// The same over int64 maps [B, nv, nz] (interval marginals: gbp_hitmap_intervals)
extern "C" gbp_status gbp_hitmap_classes_i64(int B, int nv, int nz, const int64_t* hitmap, const double* log_mean_prior, double half_width,
                                             int K, const double* means, const double* scales, double* prob, int32_t* best, double* best_p,
                                             void* stream)
{
    return hitmap_classes<long long>(B, nv, nz, (const long long*)hitmap, log_mean_prior, half_width, K, means, scales, prob, best, best_p, stream);
}

// Interval marginals of B hit maps [B, nv, nz]: out[b, v, m] = sum of hitmap[b, v, z] over lo[b, m] <= z < hi[b, m] (int64 [B, nv, M];
// lo / hi: DEVICE int32 [B, M], clamped to [0, nz] by the kernel; hi <= lo: no cells).  1 <= M <= 4096, nz <= 1024.
extern "C" gbp_status gbp_hitmap_intervals(int B, int nv, int nz, int M, const int32_t* hitmap, const int32_t* lo, const int32_t* hi,
                                           int64_t* out, void* stream)
{
    if (B < 0 || nv < 1 || nz < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_intervals: negative or zero size%s");
    if (M < 1 || M > 4096) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_intervals: M outside 1 .. 4096%s");
    if (nz > 1024) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_intervals: n_depth beyond 1024 (the row prefix lives in LDS)%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!hitmap || !lo || !hi || !out) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_intervals: NULL pointer%s");
    const int rows = (nv + hitmap::INTERVAL_ROWS - 1) / hitmap::INTERVAL_ROWS;
    if (rows > 65535) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_intervals: n_value out of range%s");
    const bool aligned = nz % 4 == 0 && ((uintptr_t)hitmap & 15) == 0;
    const int G = nz <= 256 ? 1 : (nz <= 512 ? 2 : 4);
    const size_t lds = (size_t)(256 * G + 1) * sizeof(long long) + (size_t)2 * M * sizeof(int);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(B, rows), dim3(64), lds, (hipStream_t)stream, nv, nz, M, hitmap, lo, hi, (long long*)out);
    };
    if (G == 1) { if (aligned) launch(hitmap::k_hitmap_intervals<1, true>); else launch(hitmap::k_hitmap_intervals<1, false>); }
    else if (G == 2) { if (aligned) launch(hitmap::k_hitmap_intervals<2, true>); else launch(hitmap::k_hitmap_intervals<2, false>); }
    else { if (aligned) launch(hitmap::k_hitmap_intervals<4, true>); else launch(hitmap::k_hitmap_intervals<4, false>); }
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// Replicate chains: the S * C hit maps [S * C, nv, nz] (row s * C + c: replicate c of sounding s) pooled over the chains with
// use[s, c] != 0 (DEVICE int32 [S, C]) -> pooled [S, nv, nz], and per depth cell n_used, chain_mean [S, C, nz], rhat and jsd [S, nz]
// (csrc/gbp_hitmap.h k_hitmap_pool).  2 <= C <= 8.
extern "C" gbp_status gbp_hitmap_pool(int S, int C, int nv, int nz, const int32_t* hitmap, const int32_t* use, double half_width,
                                      int32_t* pooled, int32_t* n_used, double* chain_mean, double* rhat, double* jsd, void* stream)
{
    if (S < 0 || nv < 1 || nz < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_pool: negative or zero size%s");
    if (C < 2 || C > 8) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_pool: C outside 2 .. 8%s");
    if (S == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!hitmap || !use || !pooled || !n_used || !chain_mean || !rhat || !jsd)
        return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_pool: NULL pointer%s");
    if ((int64_t)S * nz > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_pool: S * n_depth out of range%s");
    if ((nz + 255) / 256 > 65535) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_pool: n_depth out of range%s");
    const dim3 grid(S, (nz + 255) / 256);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, C, nv, nz, hitmap, use, half_width, pooled, n_used, chain_mean, rhat,
                           jsd);
    };
    if (C <= 2) launch(hitmap::k_hitmap_pool<2>);
    else if (C <= 4) launch(hitmap::k_hitmap_pool<4>);
    else launch(hitmap::k_hitmap_pool<8>);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// Local mixture fits of B hit maps [B, nv, nz]: every stage K = 1 .. Kmax of the rule of DESIGN.md 3.16 for every column in one launch
// (csrc/gbp_hitmap.h k_hitmap_mixture) -> weight / mean / sd [B, Kmax (Kmax + 1) / 2, nz], loglik / ll_change [B, Kmax, nz] and misfit
// [B, Kmax, 2, nz].  T: the maps' count type.
template <typename T>
static gbp_status hitmap_mixture(int B, int nv, int nz, const T* hitmap, double half_width, int Kmax, int n_iter, double reg, double* weight,
                                 double* mean, double* sd, double* loglik, double* ll_change, double* misfit, void* stream)
{
    if (B < 0 || nv < 1 || nz < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: negative or zero size%s");
    if (nv > hitmap::MIXTURE_MAX_ROWS)
        return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: n_value beyond 4096 (a wave's non-empty rows are a 64 x 64-bit mask)%s");
    if (Kmax < 1 || Kmax > 4) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: Kmax outside 1 .. 4%s");
    if (n_iter < 1 || n_iter > 10000) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: n_iter outside 1 .. 10000%s");
    if (!(std::isfinite(reg) && reg > 0.0)) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: reg must be finite and positive%s");
    if (!(std::isfinite(half_width) && half_width > 0.0))
        return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: half_width must be finite and positive%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!hitmap || !weight || !mean || !sd || !loglik || !ll_change || !misfit)
        return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: NULL pointer%s");
    if ((int64_t)B * nz > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: B * n_depth out of range%s");
    if ((nz + 255) / 256 > 65535) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_mixture: n_depth out of range%s");
    const hitmap::MixtureOut out = {weight, mean, sd, loglik, ll_change, misfit};
    hipLaunchKernelGGL(hitmap::k_hitmap_mixture<T>, dim3(B, (nz + 255) / 256), dim3(256), 0, (hipStream_t)stream, nv, nz, hitmap, half_width, Kmax,
                       n_iter, reg, out);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

extern "C" gbp_status gbp_hitmap_mixture(int B, int nv, int nz, const int32_t* hitmap, double half_width, int Kmax, int n_iter, double reg,
                                         double* weight, double* mean, double* sd, double* loglik, double* ll_change, double* misfit,
                                         void* stream)
{
    return hitmap_mixture<int>(B, nv, nz, hitmap, half_width, Kmax, n_iter, reg, weight, mean, sd, loglik, ll_change, misfit, stream);
}

// The same over int64 maps [B, nv, nz] (interval marginals: gbp_hitmap_intervals)
extern "C" gbp_status gbp_hitmap_mixture_i64(int B, int nv, int nz, const int64_t* hitmap, double half_width, int Kmax, int n_iter, double reg,
                                             double* weight, double* mean, double* sd, double* loglik, double* ll_change, double* misfit,
                                             void* stream)
{
    return hitmap_mixture<long long>(B, nv, nz, (const long long*)hitmap, half_width, Kmax, n_iter, reg, weight, mean, sd, loglik, ll_change,
                                     misfit, stream);
}

// The hit maps' rows (M = nv * nz cells each) as runs.  Call with start == NULL to COUNT (counts[B] <- runs per row), build the
// exclusive prefix ptr[B + 1] of the counts, allocate ptr[B] entries, then call again with ptr / start / value to WRITE.
extern "C" gbp_status gbp_hitmap_runs(int B, int64_t M, const int32_t* hitmap, int64_t* counts, const int64_t* ptr, int32_t* start,
                                      int32_t* value, void* stream)
{
    if (B == 0) return GBP_OK;
    if (B < 0 || M < 1 || M > 0x7fffffff || !hitmap) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_runs: NULL pointer or size out of range%s");
    static_assert(sizeof(long long) == sizeof(int64_t), "int64_t is long long here");
    if (start == nullptr) {
        if (!counts) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_runs: counts is NULL%s");
        hipLaunchKernelGGL(hitmap::k_hitmap_runs<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, (long long)M, hitmap, (long long*)counts,
                           (const long long*)nullptr, (int*)nullptr, (int*)nullptr);
    } else {
        if (!ptr || !value) return fail(GBP_ERR_INVALID_ARG, "gbp_hitmap_runs: ptr / value is NULL%s");
        hipLaunchKernelGGL(hitmap::k_hitmap_runs<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, (long long)M, hitmap, (long long*)nullptr,
                           (const long long*)ptr, start, value);
    }
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// [host] rows of a hit map held as runs -> one zlib stream per row (see gbp_hostpack.h); no device work
extern "C" gbp_status gbp_runs_to_zlib(int n_rows, int64_t cells_per_row, const int64_t* ptr, const int32_t* start, const int32_t* value,
                                       uint8_t* out, int64_t out_capacity, int64_t* out_ptr)
{
    if (n_rows < 0 || cells_per_row < 1 || !ptr || !out || !out_ptr || out_capacity < 0 || (n_rows > 0 && (!start || !value)))
        return fail(GBP_ERR_INVALID_ARG, "gbp_runs_to_zlib: NULL pointer or non-positive size%s");
    int64_t pos = 0;
    out_ptr[0] = 0;
    for (int r = 0; r < n_rows; ++r) {
        const int64_t a = ptr[r], b = ptr[r + 1];
        if (b <= a || start[a] != 0) return fail(GBP_ERR_INVALID_ARG, "gbp_runs_to_zlib: every row needs a first run starting at cell 0%s");
        for (int64_t q = a + 1; q < b; ++q)
            if (start[q] <= start[q - 1] || start[q] >= cells_per_row) return fail(GBP_ERR_INVALID_ARG, "gbp_runs_to_zlib: run starts must increase within the row%s");
        const size_t n = hostpack::row_to_zlib(cells_per_row, b - a, start + a, value + a, out + pos, (size_t)(out_capacity - pos));
        if (n == 0) return fail(GBP_ERR_INVALID_ARG, "gbp_runs_to_zlib: output buffer too small%s");
        pos += (int64_t)n;
        out_ptr[r + 1] = pos;
    }
    return GBP_OK;
}

// Realisations of a posterior ensemble on a depth axis (csrc/gbp_ensemble.h k_ensemble_raster): out[b, r, c] = the conductivity of the
// layer of slot slots[r] of chain b that holds z[c] -- layer = #{l < k - 1 : edges[l] <= z[c]}, the hit map's rule; the stored double
// bit for bit; a row of NaN for an empty slot (or one outside 0 .. n_ensemble - 1).  slots: DEVICE int32 [R], any order, repeats
// allowed; z: DEVICE [n_depth].  K <= 64 (a slot's rows sit one entry per lane).
extern "C" gbp_status gbp_ensemble_raster(int B, int n_ensemble, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                          int R, const int32_t* slots, int n_depth, const double* z, double* out, void* stream)
{
    if (B < 0 || n_ensemble < 1 || R < 1 || n_depth < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_raster: negative or zero size%s");
    if (n_ensemble > 4096) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_raster: n_ensemble outside 1 .. 4096%s");
    if (K < 1 || K > 64) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_raster: K outside 1 .. 64%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!ens_k || !ens_edges || !ens_sigma || !slots || !z || !out) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_raster: NULL pointer%s");
    const int64_t rows = (int64_t)B * R;
    if ((rows + 3) / 4 > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_raster: B * R out of range%s");
    const dim3 grid((unsigned)((rows + 3) / 4));
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, (long long)rows, n_ensemble, K, R, n_depth, ens_k, ens_edges, ens_sigma,
                           slots, z, out);
    };
    if (n_depth <= 64) launch(ensemble::k_ensemble_raster<1>);
    else if (n_depth <= 128) launch(ensemble::k_ensemble_raster<2>);
    else launch(ensemble::k_ensemble_raster<4>);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// Any posterior the sampler could have binned, after the fact (csrc/gbp_ensemble.h k_ensemble_rebin): every filled slot of every chain
// is added with weight 1 by the sampler's own accumulators to outputs this entry zeroes first -- hitmap int32 [B, n_value, n_depth]
// (NULL: none) on the axes given, unit_hist int32 [B, Q, n_value, n_units] for unit_z [B, n_units, 2] (n_units == 0: none), first_hist
// int32 [B, n_first, n_depth] and first_none [B, n_first] (n_first == 0: none; thresholds / directions: HOST arrays).
extern "C" gbp_status gbp_ensemble_rebin(int B, int n_ensemble, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                         const double* log_mean_prior, int n_value, double value_half_width, int n_depth, double depth_bin_width,
                                         int32_t* hitmap, int n_units, int unit_kinds, const double* unit_z, int32_t* unit_hist, int n_first,
                                         const double* first_threshold, const int32_t* first_direction, int32_t* first_hist,
                                         int32_t* first_none, void* stream)
{
    if (B < 0 || n_ensemble < 1 || n_value < 1 || n_depth < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: negative or zero size%s");
    if (n_ensemble > 4096) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: n_ensemble outside 1 .. 4096%s");
    if (K < 1 || K > 64) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: K outside 1 .. 64%s");
    if (!(std::isfinite(value_half_width) && value_half_width > 0.0) || !(std::isfinite(depth_bin_width) && depth_bin_width > 0.0))
        return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: value_half_width and depth_bin_width must be finite and positive%s");
    if (n_units < 0 || n_units > 16 || n_first < 0 || n_first > 4) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: n_units outside 0 .. 16 or n_first outside 0 .. 4%s");
    if (n_units > 0 && (unit_kinds < 1 || unit_kinds > 3)) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: unit_kinds must be 1, 2 or 3%s");
    if (n_first > 0 && (!first_threshold || !first_direction)) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: first_threshold / first_direction NULL%s");
    for (int q = 0; q < n_first; ++q) {
        if (!(std::isfinite(first_threshold[q]) && first_threshold[q] > 0.0)) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: first_threshold must be finite and positive%s");
        if (first_direction[q] != 1 && first_direction[q] != -1) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: first_direction must be +1 or -1%s");
    }
    if (!hitmap && n_units == 0 && n_first == 0) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: nothing to compute (no hitmap, no units, no thresholds)%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!ens_k || !ens_edges || !ens_sigma || !log_mean_prior || (n_units > 0 && (!unit_z || !unit_hist)) || (n_first > 0 && (!first_hist || !first_none)))
        return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_rebin: NULL pointer%s");
    gbp_rj_options o = {};
    o.max_layers = K; o.n_ensemble = n_ensemble; o.ensemble_thin = 1;
    o.n_value_bins = n_value; o.value_half_width = value_half_width; o.n_depth_bins = n_depth; o.depth_bin_width = depth_bin_width;
    o.n_units = n_units; o.unit_kinds = n_units > 0 ? unit_kinds : 0; o.n_first = n_first;
    for (int q = 0; q < n_first; ++q) { o.first_threshold[q] = first_threshold[q]; o.first_direction[q] = first_direction[q]; }
    rj::RjOpt x = {};                              // (the logarithms of extend() belong to the moves: the accumulators read none)
    static_cast<gbp_rj_options&>(x) = o;
    gbp_rj_chains c = {};
    c.B = B; c.log_mean_prior = log_mean_prior;
    c.ens_k = const_cast<int32_t*>(ens_k); c.ens_edges = const_cast<double*>(ens_edges); c.ens_sigma = const_cast<double*>(ens_sigma);
    c.hitmap = hitmap;
    if (n_units > 0) { c.unit_z = unit_z; c.unit_hist = unit_hist; }
    if (n_first > 0) { c.first_hist = first_hist; c.first_none = first_none; }
    const size_t nq = (size_t)((o.unit_kinds & 1) + ((o.unit_kinds >> 1) & 1));
    if (hitmap) GBP_HIP(hipMemsetAsync(hitmap, 0, (size_t)B * n_value * n_depth * sizeof(int32_t), (hipStream_t)stream));
    if (n_units > 0) GBP_HIP(hipMemsetAsync(unit_hist, 0, (size_t)B * nq * n_value * n_units * sizeof(int32_t), (hipStream_t)stream));
    if (n_first > 0) {
        GBP_HIP(hipMemsetAsync(first_hist, 0, (size_t)B * n_first * n_depth * sizeof(int32_t), (hipStream_t)stream));
        GBP_HIP(hipMemsetAsync(first_none, 0, (size_t)B * n_first * sizeof(int32_t), (hipStream_t)stream));
    }
    hipLaunchKernelGGL(ensemble::k_ensemble_rebin, dim3(B), dim3(64), 0, (hipStream_t)stream, x, c);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// The refusals the entries on a regularly spaced series share (csrc/gbp_ensemble_series.h), in the order a bad call meets them.  The
// launcher's own: a.reach outside lo .. hi, refused with its literal `refusal` (one %s: the entry), and `outputs`, its output pointers
// are there.  B == 0 passes before any pointer is looked at (an empty block: empty device arrays have no address): a launcher returns on it too.
static gbp_status series_check(const char* entry, int source, int B, const ensemble::SeriesArgs& a, int lo, int hi, const char* refusal, bool outputs)
{
    if (B < 0 || a.n_rows < 1 || a.V < 1) return fail(GBP_ERR_INVALID_ARG, "%s: negative or zero size", entry);
    if (a.n_rows > 32768) return fail(GBP_ERR_INVALID_ARG, "%s: more than 32 768 rows", entry);
    if (a.reach < lo || a.reach > hi) return fail(GBP_ERR_INVALID_ARG, refusal, entry);
    if (a.M_max < 1 || a.M_max > ensemble::SERIES_MAX_M) return fail(GBP_ERR_INVALID_ARG, "%s: M_max outside 1 .. 16", entry);
    if (source == ensemble::SERIES_RASTER && (a.K < 1 || a.K > 64)) return fail(GBP_ERR_INVALID_ARG, "%s: K outside 1 .. 64", entry);
    if (B == 0) return GBP_OK;
    const bool inputs = source == ensemble::SERIES_RASTER ? a.ens_k && a.ens_edges && a.ens_sigma && a.z : a.x != nullptr;
    if (!inputs || !outputs || !a.seg_start || !a.seg_m || !a.seg_n) return fail(GBP_ERR_INVALID_ARG, "%s: NULL pointer", entry);
    return GBP_OK;
}

// Chain diagnostics (csrc/gbp_ensemble_diag.h k_series_diagnostics; the rule: include/geobipy_amd.h): one workgroup per (sounding, 64
// variables).
static gbp_status series_diagnostics_launch(const char* entry, int source, int B, ensemble::DiagArgs a, void* stream)
{
    const gbp_status status = series_check(entry, source, B, a, 1, 255, "%s: max_lag outside 1 .. 255", a.stats && a.pairs);
    if (status != GBP_OK || B == 0) return status;
    const int64_t blocks = (int64_t)B * ((a.V + 63) / 64);
    if (blocks > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "%s: B * tiles out of range", entry);
    const int lds = (int)ensemble::DIAG_LDS_BYTES;
    auto launch = [&](auto kern) -> gbp_status {
        static std::atomic<bool> allowed[64];      // per instantiation (the lambda's body is one per kernel) and device: asked for once
        int dev = 0;
        GBP_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !allowed[dev].load(std::memory_order_acquire)) {
            GBP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            if (dev >= 0 && dev < 64) allowed[dev].store(true, std::memory_order_release);
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(ensemble::DIAG_WAVES * 64), (size_t)lds, (hipStream_t)stream, a);
        GBP_HIP(hipGetLastError());
        return GBP_OK;
    };
    return source == ensemble::SERIES_RASTER ? launch(ensemble::k_series_diagnostics<ensemble::SERIES_RASTER>)
                                             : launch(ensemble::k_series_diagnostics<ensemble::SERIES_PLAIN>);
}

extern "C" gbp_status gbp_series_diagnostics(int B, int n_rows, int V, const double* x, int M_max, const int32_t* seg_start, const int32_t* seg_m,
                                             const int32_t* seg_n, int max_lag, double* stats, int32_t* pairs, double* rho, void* stream)
{
    const ensemble::DiagArgs a = {{n_rows, V, x, 0, nullptr, nullptr, nullptr, nullptr, M_max, max_lag, seg_start, seg_m, seg_n}, stats, pairs, rho};
    return series_diagnostics_launch("gbp_series_diagnostics", ensemble::SERIES_PLAIN, B, a, stream);
}

extern "C" gbp_status gbp_ensemble_diagnostics(int B, int n_slots, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                               int n_depth, const double* z, int M_max, const int32_t* seg_start, const int32_t* seg_m,
                                               const int32_t* seg_n, int max_lag, double* stats, int32_t* pairs, double* rho, void* stream)
{
    const ensemble::DiagArgs a = {{n_slots, n_depth, nullptr, K, ens_k, ens_edges, ens_sigma, z, M_max, max_lag, seg_start, seg_m, seg_n}, stats, pairs, rho};
    return series_diagnostics_launch("gbp_ensemble_diagnostics", ensemble::SERIES_RASTER, B, a, stream);
}

#include "gbp_ensemble_ranks.h"

// Ranks within columns (csrc/gbp_ensemble_ranks.h k_series_ranks; the rule: include/geobipy_amd.h): one workgroup per (sounding, tile
// of T columns), T and the padded length P from n_rows.
static gbp_status series_ranks_launch(const char* entry, int source, int B, ensemble::RankArgs a, int fold, const double* p, void* stream)
{
    using namespace ensemble;
    const gbp_status status = series_check(entry, source, B, a, 0, RANK_MAX_P, "%s: n_p outside 0 .. 16", true);
    if (status != GBP_OK) return status;
    if (a.n_rows > RANK_MAX_ROWS) return fail(GBP_ERR_INVALID_ARG, "%s: more than 16 384 rows", entry);
    if (a.reach > 0 && !p) return fail(GBP_ERR_INVALID_ARG, "%s: NULL pointer", entry);
    for (int q = 0; q < a.reach; ++q) {
        if (!(std::isfinite(p[q]) && p[q] >= 0.0 && p[q] <= 1.0)) return fail(GBP_ERR_INVALID_ARG, "%s: a probability outside [0, 1]", entry);
        a.p[q] = p[q];
    }
    if ((a.less == nullptr) != (a.leq == nullptr)) return fail(GBP_ERR_INVALID_ARG, "%s: less and leq come as a pair", entry);
    if (a.order != nullptr && a.reach == 0) a.order = nullptr;      // (nothing to write)
    int P = 1;
    while (P < a.n_rows) P <<= 1;
    const int T = std::min(64, RANK_TILE_DOUBLES / P);
    const int64_t blocks = (int64_t)B * ((a.V + T - 1) / T);
    if (blocks * RANK_THREADS > 0xffffffffLL)                       // (a dispatch counts its work-items in 32 bits)
        return fail(GBP_ERR_INVALID_ARG, "%s: B * column tiles out of range (more than 2^32 - 1 threads)", entry);
    if (B == 0 || (!a.less && !a.order && !a.x_out)) return GBP_OK;
    a.T = T;
    a.P = P;
    const size_t lds = rank_lds_bytes(T, P);
    auto launch = [&](auto kern) -> gbp_status {
        static std::atomic<bool> allowed[64];      // per instantiation and device: asked for once, for the largest tile
        int dev = 0;
        GBP_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !allowed[dev].load(std::memory_order_acquire)) {
            GBP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rank_lds_bytes(64, RANK_TILE_DOUBLES / 64)));
            if (dev >= 0 && dev < 64) allowed[dev].store(true, std::memory_order_release);
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(RANK_THREADS), lds, (hipStream_t)stream, a);
        GBP_HIP(hipGetLastError());
        return GBP_OK;
    };
    if (source == SERIES_RASTER) return fold ? launch(k_series_ranks<SERIES_RASTER, true>) : launch(k_series_ranks<SERIES_RASTER, false>);
    return fold ? launch(k_series_ranks<SERIES_PLAIN, true>) : launch(k_series_ranks<SERIES_PLAIN, false>);
}

extern "C" gbp_status gbp_series_ranks(int B, int n_rows, int V, const double* x, int M_max, const int32_t* seg_start, const int32_t* seg_m,
                                       const int32_t* seg_n, int fold, int n_p, const double* p, int32_t* less, int32_t* leq, double* order,
                                       double* x_out, void* stream)
{
    const ensemble::RankArgs a = {{n_rows, V, x, 0, nullptr, nullptr, nullptr, nullptr, M_max, n_p, seg_start, seg_m, seg_n}, less, leq, order, x_out, 0, 0, {}};
    return series_ranks_launch("gbp_series_ranks", ensemble::SERIES_PLAIN, B, a, fold, p, stream);
}

extern "C" gbp_status gbp_ensemble_ranks(int B, int n_slots, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                         int n_depth, const double* z, int M_max, const int32_t* seg_start, const int32_t* seg_m,
                                         const int32_t* seg_n, int fold, int n_p, const double* p, int32_t* less, int32_t* leq, double* order,
                                         double* x_out, void* stream)
{
    const ensemble::RankArgs a = {{n_slots, n_depth, nullptr, K, ens_k, ens_edges, ens_sigma, z, M_max, n_p, seg_start, seg_m, seg_n}, less, leq, order, x_out, 0, 0, {}};
    return series_ranks_launch("gbp_ensemble_ranks", ensemble::SERIES_RASTER, B, a, fold, p, stream);
}

#include "gbp_ensemble_weighted.h"

// Weighted products within columns (csrc/gbp_ensemble_weighted.h k_series_weighted; the rule: include/geobipy_amd.h): one workgroup per
// (sounding, tile of T columns), T from the power of two >= n.
static gbp_status series_weighted_launch(const char* entry, int source, int B, ensemble::WeightedArgs a, const double* p, const double* thr, void* stream)
{
    using namespace ensemble;
    if (B < 0 || a.n_rows < 1 || a.V < 1) return fail(GBP_ERR_INVALID_ARG, "%s: negative or zero size", entry);
    if (a.n < 1 || a.n > WGT_MAX_ROWS) return fail(GBP_ERR_INVALID_ARG, "%s: n outside 1 .. 4096", entry);
    if (source == SERIES_RASTER && (a.K < 1 || a.K > 64)) return fail(GBP_ERR_INVALID_ARG, "%s: K outside 1 .. 64", entry);
    if (a.n_p < 0 || a.n_p > WGT_MAX_P) return fail(GBP_ERR_INVALID_ARG, "%s: n_p outside 0 .. 16", entry);
    if (a.n_t < 0 || a.n_t > WGT_MAX_T) return fail(GBP_ERR_INVALID_ARG, "%s: n_t outside 0 .. 8", entry);
    if ((a.n_p > 0 && !p) || (a.n_t > 0 && !thr)) return fail(GBP_ERR_INVALID_ARG, "%s: NULL pointer", entry);
    for (int i = 0; i < a.n_p; ++i) {
        if (!(std::isfinite(p[i]) && p[i] >= 0.0 && p[i] <= 1.0)) return fail(GBP_ERR_INVALID_ARG, "%s: a probability outside [0, 1]", entry);
        a.p[i] = p[i];
    }
    for (int j = 0; j < a.n_t; ++j) {
        if (!std::isfinite(thr[j])) return fail(GBP_ERR_INVALID_ARG, "%s: a threshold that is not finite", entry);
        a.thr[j] = thr[j];
    }
    int P = 1;
    while (P < a.n) P <<= 1;
    const int T = std::min(64, WGT_TILE / P);
    const int64_t blocks = (int64_t)B * ((a.V + T - 1) / T);
    if (blocks * WGT_THREADS > 0xffffffffLL)                        // (a dispatch counts its work-items in 32 bits)
        return fail(GBP_ERR_INVALID_ARG, "%s: B * column tiles out of range (more than 2^32 - 1 threads)", entry);
    if (B == 0) return GBP_OK;                                      // (an empty block: empty device arrays have no address)
    const bool inputs = source == SERIES_RASTER ? a.ens_k && a.ens_edges && a.ens_sigma && a.z : a.x != nullptr;
    if (!inputs || !a.rows || !a.n_used || !a.q || !a.total) return fail(GBP_ERR_INVALID_ARG, "%s: NULL pointer", entry);
    a.T = T;
    a.P = P;
    const size_t lds = weighted_lds_bytes(T, P);
    auto launch = [&](auto kern) -> gbp_status {
        static std::atomic<bool> allowed[64];      // per instantiation and device: asked for once, for the largest tile
        int dev = 0;
        GBP_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !allowed[dev].load(std::memory_order_acquire)) {
            GBP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)weighted_lds_bytes(64, WGT_TILE / 64)));
            if (dev >= 0 && dev < 64) allowed[dev].store(true, std::memory_order_release);
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(WGT_THREADS), lds, (hipStream_t)stream, a);
        GBP_HIP(hipGetLastError());
        return GBP_OK;
    };
    return source == SERIES_RASTER ? launch(k_series_weighted<SERIES_RASTER>) : launch(k_series_weighted<SERIES_PLAIN>);
}

extern "C" gbp_status gbp_series_weighted(int B, int n_rows, int V, const double* x, int n, const int32_t* rows, const int32_t* n_used, const int64_t* q,
                                          int n_p, const double* p, int n_t, const double* thr, int64_t* total, double* quantile, int64_t* above,
                                          double* stats, void* stream)
{
    const ensemble::WeightedArgs a = {{n_rows, V, x, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr}, n, rows, n_used,
                                      (const long long*)q, n_p, n_t, (long long*)total, quantile, (long long*)above, stats, 0, 0, {}, {}};
    return series_weighted_launch("gbp_series_weighted", ensemble::SERIES_PLAIN, B, a, p, thr, stream);
}

extern "C" gbp_status gbp_ensemble_weighted(int B, int n_slots, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                            int n_depth, const double* z, int n, const int32_t* rows, const int32_t* n_used, const int64_t* q,
                                            int n_p, const double* p, int n_t, const double* thr, int64_t* total, double* quantile,
                                            int64_t* above, double* stats, void* stream)
{
    const ensemble::WeightedArgs a = {{n_slots, n_depth, nullptr, K, ens_k, ens_edges, ens_sigma, z, 0, 0, nullptr, nullptr, nullptr}, n, rows, n_used,
                                      (const long long*)q, n_p, n_t, (long long*)total, quantile, (long long*)above, stats, 0, 0, {}, {}};
    return series_weighted_launch("gbp_ensemble_weighted", ensemble::SERIES_RASTER, B, a, p, thr, stream);
}

#include "gbp_ensemble_corr.h"

// Correlation between variables (csrc/gbp_ensemble_corr.h; the rule: include/geobipy_amd.h): the moments, the MFMA kernel, then the two
// streaming kernels of the finish, in stream order.
static gbp_status series_correlation_launch(const char* entry, int source, int B, ensemble::CorrArgs a, int normalise, void* stream)
{
    using namespace ensemble;
    const int W = a.reach;
    const gbp_status status = series_check(entry, source, B, a, 0, a.V - 1, "%s: band_width outside 0 .. V - 1", a.stats && a.band);
    if (status != GBP_OK || B == 0) return status;
    const int ntiles = (a.V + 15) / 16, nstrips = (ntiles + CORR_WAVES - 1) / CORR_WAVES;
    const int DJ = (W + 15) / 16 + 1, npanels = (DJ + CORR_NACC - 1) / CORR_NACC;
    const int64_t moment_blocks = (int64_t)B * ((a.V + 63) / 64), blocks = (int64_t)B * nstrips * npanels;
    const int64_t entries = (int64_t)B * a.V * (W + 1), finish_blocks = (entries + 255) / 256;
    if (moment_blocks > 0x7fffffffLL || blocks > 0x7fffffffLL || finish_blocks > 0x7fffffffLL)
        return fail(GBP_ERR_INVALID_ARG, "%s: B * V * (band_width + 1) out of range", entry);
    const int ncol = (std::min(DJ, CORR_NACC) + CORR_WAVES - 1) * 16 + (npanels > 1 ? CORR_WAVES * 16 : 0);      // the widest staged row
    const size_t lds = (size_t)CORR_CH * (ncol + ((ncol & 31) == 0 ? 16 : 0)) * sizeof(double);                    // <= CORR_LDS_BYTES < 64 KiB
    hipStream_t s = (hipStream_t)stream;
    if (source == SERIES_RASTER) {
        hipLaunchKernelGGL(k_series_moments<SERIES_RASTER>, dim3((unsigned)moment_blocks), dim3(CORR_WAVES * 64), 0, s, a);
        hipLaunchKernelGGL(k_series_correlation<SERIES_RASTER>, dim3((unsigned)blocks), dim3(CORR_WAVES * 64), lds, s, a, npanels);
    } else {
        hipLaunchKernelGGL(k_series_moments<SERIES_PLAIN>, dim3((unsigned)moment_blocks), dim3(CORR_WAVES * 64), 0, s, a);
        hipLaunchKernelGGL(k_series_correlation<SERIES_PLAIN>, dim3((unsigned)blocks), dim3(CORR_WAVES * 64), lds, s, a, npanels);
    }
    const size_t cells = (size_t)B * a.V;
    hipLaunchKernelGGL(k_correlation_sd, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, cells, a.V, W, a.band, a.stats);
    hipLaunchKernelGGL(k_correlation_finish, dim3((unsigned)finish_blocks), dim3(256), 0, s, (size_t)entries, a.V, W, normalise, a.stats, a.band);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

extern "C" gbp_status gbp_series_correlation(int B, int n_rows, int V, const double* x, int M_max, const int32_t* seg_start, const int32_t* seg_m,
                                             const int32_t* seg_n, int band_width, int normalise, double* stats, double* band, void* stream)
{
    const ensemble::CorrArgs a = {{n_rows, V, x, 0, nullptr, nullptr, nullptr, nullptr, M_max, band_width, seg_start, seg_m, seg_n}, stats, band};
    return series_correlation_launch("gbp_series_correlation", ensemble::SERIES_PLAIN, B, a, normalise, stream);
}

extern "C" gbp_status gbp_ensemble_correlation(int B, int n_slots, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                               int n_depth, const double* z, int M_max, const int32_t* seg_start, const int32_t* seg_m,
                                               const int32_t* seg_n, int band_width, int normalise, double* stats, double* band, void* stream)
{
    const ensemble::CorrArgs a = {{n_slots, n_depth, nullptr, K, ens_k, ens_edges, ens_sigma, z, M_max, band_width, seg_start, seg_m, seg_n}, stats, band};
    return series_correlation_launch("gbp_ensemble_correlation", ensemble::SERIES_RASTER, B, a, normalise, stream);
}

extern "C" gbp_status gbp_band_runs(int B, int V, int band_width, const double* band, double threshold, int32_t* up, int32_t* down,
                                    uint8_t* closed, void* stream)
{
    if (B < 0 || V < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_band_runs: negative or zero size%s");
    if (band_width < 0 || band_width > V - 1) return fail(GBP_ERR_INVALID_ARG, "gbp_band_runs: band_width outside 0 .. V - 1%s");
    if (threshold != threshold) return fail(GBP_ERR_INVALID_ARG, "gbp_band_runs: threshold is NaN%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!band || !up || !down || !closed) return fail(GBP_ERR_INVALID_ARG, "gbp_band_runs: NULL pointer%s");
    const size_t cells = (size_t)B * V;
    if ((cells + 255) / 256 > 0x7fffffffull) return fail(GBP_ERR_INVALID_ARG, "gbp_band_runs: B * V out of range%s");
    hipLaunchKernelGGL(ensemble::k_band_runs, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cells, V, band_width, band,
                       threshold, up, down, closed);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

#include "gbp_ensemble_families.h"

// Families of kept models (csrc/gbp_ensemble_families.h; the rules: include/geobipy_amd.h): the distance between layered models ...
extern "C" gbp_status gbp_ensemble_distance(int B, int n_slots, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                            int n, const int32_t* rows, double z0, double z1, int measure, int log10, int squared, double* dist,
                                            void* stream)
{
    using namespace ensemble;
    if (B < 0 || n_slots < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: negative or zero size%s");
    if (n < 1 || n > 4096) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: n outside 1 .. 4096%s");
    if (K < 1 || K > 64) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: K outside 1 .. 64%s");
    if (!std::isfinite(z0) || !std::isfinite(z1) || z0 < 0.0 || z1 <= z0)
        return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: the window needs finite bounds with 0 <= z0 < z1%s");
    if (measure != 0 && measure != 1) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: measure must be 0 (linear) or 1 (log)%s");
    if (measure == 1 && z0 == 0.0) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: the log measure needs z0 > 0%s");
    const int nt = (n + FAM_TILE - 1) / FAM_TILE, ntp = nt * (nt + 1) / 2;
    if ((int64_t)B * ntp * FAM_THREADS > 0xffffffffLL)             // (a dispatch counts its work-items in 32 bits)
        return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: B * tile pairs out of range (more than 2^32 - 1 threads)%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!ens_k || !ens_edges || !ens_sigma || !rows || !dist) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_distance: NULL pointer%s");
    const double mu = measure == 1 ? std::log1p((z1 - z0) / z0) : z1 - z0;      // (ln(z1 / z0), as the kernel takes a segment's: a narrow deep window)
    const DistanceArgs a = {n_slots, K, n, ens_k, ens_edges, ens_sigma, rows, z0, z1, 1.0 / mu, log10 ? 1 : 0, squared ? 1 : 0, ntp, dist};
    const dim3 grid((unsigned)((int64_t)B * ntp));
    if (measure == 1) hipLaunchKernelGGL(k_layered_distance<true>, grid, dim3(FAM_THREADS), distance_lds_bytes(K), (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_layered_distance<false>, grid, dim3(FAM_THREADS), distance_lds_bytes(K), (hipStream_t)stream, a);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// ... the same distance between the models of a sounding and those of its partner sounding: all nt x nt tiles ...
extern "C" gbp_status gbp_ensemble_cross_distance(int S, int n_slots, int K, const int32_t* ens_k, const double* ens_edges,
                                                  const double* ens_sigma, int n, const int32_t* rows, const int32_t* partner, double z0,
                                                  double z1, int measure, int log10, int squared, double* dist, void* stream)
{
    using namespace ensemble;
    if (S < 0 || n_slots < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: negative or zero size%s");
    if (n < 1 || n > 4096) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: n outside 1 .. 4096%s");
    if (K < 1 || K > 64) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: K outside 1 .. 64%s");
    if (!std::isfinite(z0) || !std::isfinite(z1) || z0 < 0.0 || z1 <= z0)
        return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: the window needs finite bounds with 0 <= z0 < z1%s");
    if (measure != 0 && measure != 1) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: measure must be 0 (linear) or 1 (log)%s");
    if (measure == 1 && z0 == 0.0) return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: the log measure needs z0 > 0%s");
    const int nt = (n + FAM_TILE - 1) / FAM_TILE, nt2 = nt * nt;
    if ((int64_t)S * nt2 * FAM_THREADS > 0xffffffffLL)             // (a dispatch counts its work-items in 32 bits)
        return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: S * tiles out of range (more than 2^32 - 1 threads)%s");
    if (S == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!ens_k || !ens_edges || !ens_sigma || !rows || !partner || !dist)
        return fail(GBP_ERR_INVALID_ARG, "gbp_ensemble_cross_distance: NULL pointer%s");
    const double mu = measure == 1 ? std::log1p((z1 - z0) / z0) : z1 - z0;      // (as gbp_ensemble_distance takes it)
    const CrossDistanceArgs a = {S, n_slots, K, n, ens_k, ens_edges, ens_sigma, rows, partner, z0, z1, 1.0 / mu, log10 ? 1 : 0, squared ? 1 : 0,
                                 nt2, dist};
    const dim3 grid((unsigned)((int64_t)S * nt2));
    if (measure == 1) hipLaunchKernelGGL(k_layered_cross_distance<true>, grid, dim3(FAM_THREADS), distance_lds_bytes(K), (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_layered_cross_distance<false>, grid, dim3(FAM_THREADS), distance_lds_bytes(K), (hipStream_t)stream, a);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// ... and k-medoids on the distances, every stage of a sounding in one launch: one workgroup per sounding.
extern "C" gbp_status gbp_distance_families(int B, int n, const double* dist, const int32_t* n_used, int q_max, int max_iter, int32_t* medoid,
                                            int32_t* label, double* nearest, double* second, int32_t* iterations, uint8_t* converged,
                                            int32_t* n_found, void* stream)
{
    using namespace ensemble;
    if (B < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_distance_families: negative size%s");
    if (n < 1 || n > 4096) return fail(GBP_ERR_INVALID_ARG, "gbp_distance_families: n outside 1 .. 4096%s");
    if (q_max < 1 || q_max > FAM_MAX_Q) return fail(GBP_ERR_INVALID_ARG, "gbp_distance_families: q_max outside 1 .. 8%s");
    if (max_iter < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_distance_families: max_iter must be >= 0%s");
    if ((int64_t)B * FAM_THREADS > 0xffffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_distance_families: B out of range (more than 2^32 - 1 threads)%s");
    if (B == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!dist || !n_used || !medoid || !label || !nearest || !second || !iterations || !converged || !n_found)
        return fail(GBP_ERR_INVALID_ARG, "gbp_distance_families: NULL pointer%s");
    const FamilyArgs a = {n, q_max, max_iter, dist, n_used, medoid, label, nearest, second, iterations, converged, n_found};
    hipLaunchKernelGGL(k_distance_families, dim3((unsigned)B), dim3(FAM_THREADS), families_lds_bytes(n), (hipStream_t)stream, a);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

#include "gbp_grid.h"

// Discrete Sibson gridding (gbp_grid.h): the plan holds the geometry of one grid -- nearest sounding, D, n, and per destination pixel the
// list of the soundings its covering pixels point at, in row-major order of those pixels -- in bands of destination rows.  One band
// (the lists fit the budget): they are written once, here.  Several: the plan keeps one band's room and gbp_sibson_apply rewrites it
// band by band, so the sums and their order are the same either way.
struct gbp_sibson_plan {
    struct Band { int row0, row1, tile0, ntiles; long long base, len; };
    int device = 0, N = 0, nx = 0, ny = 0, nseg = 0;
    double max_d2 = 0.0;
    int *d_index = nullptr, *d_D = nullptr, *d_n = nullptr, *d_segmax = nullptr, *d_rowmax = nullptr, *d_order = nullptr, *d_list = nullptr;
    long long* d_ptr = nullptr;
    long long total = 0, longest = 0, capacity = 0;
    std::vector<Band> bands;
};

namespace {

const int64_t GBP_SIBSON_DEFAULT_BUDGET = (int64_t)4 << 30;

gbp_status sibson_fill(const gbp_sibson_plan* p, const gbp_sibson_plan::Band& b, hipStream_t stream)
{
    const long long cells = (long long)(b.row1 - b.row0) * p->nx;
    hipLaunchKernelGGL(grid::k_cover_walk<true>, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p->nx, p->ny, p->nseg, b.row0, b.row1,
                       p->d_D, p->d_segmax, p->d_rowmax, p->d_index, (int*)nullptr, p->d_ptr, b.base, p->d_list);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

}  // namespace

extern "C" void gbp_sibson_plan_destroy(gbp_sibson_plan* p)
{
    if (!p) return;
    for (void* d : {(void*)p->d_index, (void*)p->d_D, (void*)p->d_n, (void*)p->d_segmax, (void*)p->d_rowmax, (void*)p->d_order, (void*)p->d_list,
                    (void*)p->d_ptr})
        if (d) (void)hipFree(d);
    delete p;
}

extern "C" gbp_status gbp_sibson_plan_create_ex(int N, const double* px, const double* py, int nx, int ny, double max_distance_px2,
                                                int64_t list_budget_bytes, void* stream, gbp_sibson_plan** out)
{
    if (!out) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: out is NULL%s");
    *out = nullptr;
    if (N < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: N must be >= 1%s");
    if (nx < 1 || ny < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: nx and ny must be >= 1%s");
    if ((int64_t)nx * ny > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: nx * ny out of range (int32 pixel index)%s");
    if (!px || !py) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: NULL pointer%s");
    if (max_distance_px2 != max_distance_px2) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: max_distance_px2 is NaN (+inf for no mask)%s");
    if (list_budget_bytes < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: negative list budget%s");
    const int64_t budget = (list_budget_bytes ? list_budget_bytes : GBP_SIBSON_DEFAULT_BUDGET) / (int64_t)sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> h((size_t)2 * N);
    GBP_HIP(hipMemcpyAsync(h.data(), px, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    GBP_HIP(hipMemcpyAsync(h.data() + N, py, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    GBP_HIP(hipStreamSynchronize(st));
    for (double v : h)
        if (!std::isfinite(v)) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: non-finite pixel coordinate%s");

    gbp_sibson_plan* p = new (std::nothrow) gbp_sibson_plan();
    if (!p) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: out of host memory%s");
    const size_t P = (size_t)nx * ny;
    p->N = N; p->nx = nx; p->ny = ny; p->nseg = (nx + grid::SEG - 1) / grid::SEG; p->max_d2 = max_distance_px2;
    const int tiles_per_row = p->nseg;
    const size_t ntiles = (size_t)tiles_per_row * ny;
    std::vector<int> hn;
    std::vector<long long> hptr;
    std::vector<int> order;
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_index, P * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_D, P * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_n, P * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_segmax, ntiles * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_rowmax, (size_t)ny * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_order, ntiles * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_ptr, (P + 1) * sizeof(long long));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(grid::k_grid_nearest, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, N, px, py, nx, ny, p->d_index, p->d_D);
        hipLaunchKernelGGL(grid::k_grid_segmax, dim3(ny), dim3(64), 0, st, nx, ny, p->nseg, p->d_D, p->d_segmax, p->d_rowmax);
        hipLaunchKernelGGL(grid::k_cover_walk<false>, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, nx, ny, p->nseg, 0, ny, p->d_D,
                           p->d_segmax, p->d_rowmax, p->d_index, p->d_n, (const long long*)nullptr, 0LL, (int*)nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hn.resize(P);
        e = hipMemcpyAsync(hn.data(), p->d_n, P * sizeof(int), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        gbp_sibson_plan_destroy(p);
        return fail(GBP_ERR_HIP, "gbp_sibson_plan_create: %s", hipGetErrorString(e));
    }
    // exclusive prefix over the whole grid, bands of rows within the budget, tiles of a band longest first
    hptr.resize(P + 1);
    hptr[0] = 0;
    for (size_t q = 0; q < P; ++q) {
        hptr[q + 1] = hptr[q] + hn[q];
        p->longest = std::max(p->longest, (long long)hn[q]);
    }
    p->total = hptr[P];
    auto add_band = [&](int r0, int r1) {
        gbp_sibson_plan::Band b = {r0, r1, r0 * tiles_per_row, (r1 - r0) * tiles_per_row, hptr[(size_t)r0 * nx], 0};
        b.len = hptr[(size_t)r1 * nx] - b.base;
        p->bands.push_back(b);
        p->capacity = std::max(p->capacity, b.len);
    };
    int row0 = 0;
    long long held = 0;
    for (int i = 0; i < ny; ++i) {
        const long long row = hptr[(size_t)(i + 1) * nx] - hptr[(size_t)i * nx];
        if (row > budget) {
            gbp_sibson_plan_destroy(p);
            return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_create: one destination row's lists exceed the list budget%s");
        }
        if (i > row0 && held + row > budget) {
            add_band(row0, i);
            row0 = i;
            held = 0;
        }
        held += row;
    }
    add_band(row0, ny);
    order.resize(ntiles);
    std::vector<long long> work(ntiles);
    long long wmax = 1;
    for (size_t t = 0; t < ntiles; ++t) {
        const size_t r = t / tiles_per_row, j0 = (t % tiles_per_row) * grid::SEG, j1 = std::min((size_t)nx, j0 + grid::SEG);
        work[t] = hptr[r * nx + j1] - hptr[r * nx + j0];
        wmax = std::max(wmax, work[t]);
        order[t] = (int)t;
    }
    for (const auto& b : p->bands)                 // sixteen classes of work; neighbours stay neighbours inside a class
        std::stable_sort(order.begin() + b.tile0, order.begin() + b.tile0 + b.ntiles,
                         [&](int a, int c) { return work[a] * 16 / wmax > work[c] * 16 / wmax; });
    e = hipMalloc((void**)&p->d_list, (size_t)std::max(p->capacity, 1LL) * sizeof(int));
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_ptr, hptr.data(), (P + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_order, order.data(), ntiles * sizeof(int), hipMemcpyHostToDevice, st);
    gbp_status rc = GBP_OK;
    if (e == hipSuccess && p->bands.size() == 1) rc = sibson_fill(p, p->bands[0], st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the host arrays of the uploads die with this call)
    if (e != hipSuccess || rc != GBP_OK) {
        gbp_sibson_plan_destroy(p);
        return e != hipSuccess ? fail(GBP_ERR_HIP, "gbp_sibson_plan_create: %s", hipGetErrorString(e)) : rc;
    }
    *out = p;
    return GBP_OK;
}

extern "C" gbp_status gbp_sibson_plan_create(int N, const double* px, const double* py, int nx, int ny, double max_distance_px2, void* stream,
                                             gbp_sibson_plan** out)
{
    return gbp_sibson_plan_create_ex(N, px, py, nx, ny, max_distance_px2, 0, stream, out);
}

extern "C" gbp_status gbp_sibson_plan_query(const gbp_sibson_plan* p, int32_t* index, int32_t* distance, int32_t* count, int64_t* info, void* stream)
{
    if (!p) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_plan_query: plan is NULL%s");
    const size_t bytes = (size_t)p->nx * p->ny * sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    if (index) GBP_HIP(hipMemcpyAsync(index, p->d_index, bytes, hipMemcpyDeviceToDevice, st));
    if (distance) GBP_HIP(hipMemcpyAsync(distance, p->d_D, bytes, hipMemcpyDeviceToDevice, st));
    if (count) GBP_HIP(hipMemcpyAsync(count, p->d_n, bytes, hipMemcpyDeviceToDevice, st));
    if (info) {
        const int64_t P = (int64_t)p->nx * p->ny, ntiles = (int64_t)p->nseg * p->ny;
        info[0] = p->total;
        info[1] = p->longest;
        info[2] = (int64_t)p->bands.size();
        info[3] = 3 * P * 4 + 2 * ntiles * 4 + (int64_t)p->ny * 4 + (P + 1) * 8 + std::max(p->capacity, 1LL) * 4;
    }
    return GBP_OK;
}

extern "C" gbp_status gbp_sibson_apply(const gbp_sibson_plan* p, int C, const double* values, double* out, void* stream)
{
    if (!p) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_apply: plan is NULL%s");
    if (C < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_apply: C must be >= 1%s");
    if (!values || !out) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_apply: NULL pointer%s");
    const int64_t P = (int64_t)p->nx * p->ny, lim = 0x7fffffffffffffffLL / 8;
    const int cblocks = (C + grid::COLS - 1) / grid::COLS;
    if (cblocks > 65535 || (int64_t)C > lim / P || (int64_t)C > lim / p->N)
        return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_apply: C * nx * ny or N * C out of range%s");
    hipStream_t st = (hipStream_t)stream;
    for (const auto& b : p->bands) {
        if (p->bands.size() > 1) {
            gbp_status rc = sibson_fill(p, b, st);
            if (rc != GBP_OK) return rc;
        }
        hipLaunchKernelGGL(grid::k_sibson_gather, dim3(b.ntiles, cblocks), dim3(256), 0, st, C, p->nx, p->ny, p->nseg, p->d_order, b.tile0, p->d_ptr,
                           b.base, p->d_list, p->d_D, p->max_d2, values, out);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

// Pixel posteriors (k_sibson_pool): the hit maps of each listed pixel's cover list summed, a neighbour's value axis moved onto the nearest
// sounding's.  Every refusal comes before the launch; the pooled cells are int32, so the longest list times the caller's bound of a
// column's total must stay inside it.
extern "C" gbp_status gbp_sibson_pool(const gbp_sibson_plan* p, int n_pixels, const int32_t* pixels, int n_value, int n_depth,
                                      const int32_t* maps, const double* u, int64_t max_total, int32_t* pooled, int64_t* clipped, void* stream)
{
    if (n_pixels < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: n_pixels must be >= 0%s");
    if (n_value < 1 || n_depth < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: n_value and n_depth must be >= 1%s");
    if (n_depth > (1 << 29)) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: n_depth out of range (a row's bytes are a 32-bit lane offset)%s");
    if (max_total < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: max_total must be >= 0%s");
    if (n_pixels == 0) return GBP_OK;
    if (!p) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: plan is NULL%s");
    if (!pixels || !maps || !pooled) return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: NULL pointer%s");
    if (p->bands.size() > 1)
        return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: the plan is banded (its lists exceed the list budget); pooling needs the lists of one band%s");
    if (max_total > 0 && p->longest > 0x7fffffffLL / max_total)
        return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: longest list times max_total exceeds 2^31 - 1, a pooled int32 cell could overflow%s");
    const int cpl = n_depth > 64 ? 2 : 1;
    const int64_t tiles = ((int64_t)n_depth + 64 * cpl - 1) / (64 * cpl), lim = 0x7fffffffffffffffLL / 8;
    if ((int64_t)n_pixels * tiles > 0x7fffffffLL || (int64_t)n_value > lim / n_depth / std::max(p->N, n_pixels))
        return fail(GBP_ERR_INVALID_ARG, "gbp_sibson_pool: n_pixels * depth tiles or the maps' size out of range%s");
    hipStream_t st = (hipStream_t)stream;
    auto kernel = cpl == 2 ? grid::k_sibson_pool<2> : grid::k_sibson_pool<1>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_pixels * tiles)), dim3(256), 0, st, n_pixels, pixels, p->nx, p->ny, n_value, n_depth, (int)tiles,
                       p->d_ptr, p->d_list, p->d_index, p->d_D, p->max_d2, maps, u, pooled, (long long*)clipped);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

#include "gbp_elev.h"

// Elevation slices (gbp_elev.h): rows on the depth axis onto levels or cells of an elevation axis, one launch per call.
extern "C" gbp_status gbp_elevation_resample(int mode, int R, int K, int n_depth, const double* values, const double* surface,
                                             const double* depth_edges, int E, const double* axis, int c0, int c1, double* out, void* stream)
{
    if (mode != GBP_ELEVATION_LEVELS && mode != GBP_ELEVATION_INTERVALS)
        return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: mode must be GBP_ELEVATION_LEVELS or GBP_ELEVATION_INTERVALS%s");
    if (R < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: R must be >= 1%s");
    if (K < 1 || R % K != 0) return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: K must be >= 1 and divide R%s");
    if (n_depth < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: n_depth must be >= 1%s");
    if (n_depth > elev::MAX_DEPTH_CELLS) return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: n_depth out of range (at most 8191 depth cells)%s");
    if (E < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: E must be >= 1%s");
    if (c0 < 0 || c1 > E || c0 >= c1) return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: the column window needs 0 <= c0 < c1 <= E%s");
    if (!values || !surface || !depth_edges || !axis || !out) return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: NULL pointer%s");
    const int ncols = c1 - c0;
    const int64_t lim = 0x7fffffffffffffffLL / 8;
    const int cblocks = (ncols + elev::COLS - 1) / elev::COLS;
    if (cblocks > 65535 || (int64_t)R > lim / n_depth || (int64_t)R > lim / ncols)
        return fail(GBP_ERR_INVALID_ARG, "gbp_elevation_resample: R * n_depth or R * columns out of range%s");
    hipStream_t st = (hipStream_t)stream;
    const dim3 blocks((unsigned)(((int64_t)R + elev::ROWS - 1) / elev::ROWS), (unsigned)cblocks);
    const size_t lds = (size_t)(n_depth + 1) * sizeof(double);
    if (mode == GBP_ELEVATION_INTERVALS)
        hipLaunchKernelGGL(elev::k_elevation_resample<true>, blocks, dim3(256), lds, st, R, K, n_depth, values, surface, depth_edges, axis, c0, ncols, out);
    else
        hipLaunchKernelGGL(elev::k_elevation_resample<false>, blocks, dim3(256), lds, st, R, K, n_depth, values, surface, depth_edges, axis, c0, ncols, out);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

#include "gbp_horizon.h"

// Horizon tracking (gbp_horizon.h): one workgroup per sequence walks its Markov chain; the Viterbi launch always, the forward-backward
// launch only when the marginals are asked for.  Every refusal comes before any launch; ptr is not read on the host.
namespace {

template <int NJ>
gbp_status horizon_launch(int L, const int64_t* ptr, int S, double dz, const double* score, const double* absent_score, const double* g,
                          const double* d, double sw, uint16_t* back, int32_t* cell, double* log_score, double* marginal,
                          double* log_partition, double* scale, hipStream_t st)
{
    const size_t lds = horizon::lds_doubles(S) * sizeof(double);
    const int has_absent = absent_score ? 1 : 0;
    if (lds > 48 * 1024) {                                                  // (above the default limit of a launch's dynamic LDS)
        (void)hipFuncSetAttribute((const void*)horizon::k_horizon_viterbi<NJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void*)horizon::k_horizon_marginals<NJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(horizon::k_horizon_viterbi<NJ>, dim3((unsigned)L), dim3(horizon::THREADS), lds, st, (const long long*)ptr, S, has_absent, dz,
                       score, absent_score, g, d, sw, (unsigned short*)back, (int*)cell, log_score);
    GBP_HIP(hipGetLastError());
    if (marginal) {
        hipLaunchKernelGGL(horizon::k_horizon_marginals<NJ>, dim3((unsigned)L), dim3(horizon::THREADS), lds, st, (const long long*)ptr, S, has_absent,
                           dz, score, absent_score, g, d, sw, marginal, log_partition, scale);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

}  // namespace

extern "C" gbp_status gbp_horizon_track(int L, const int64_t* ptr, int64_t total_n, int max_n, int S, double dz, const double* score,
                                        const double* absent_score, const double* g, const double* d, double switch_cost, uint16_t* back,
                                        int32_t* cell, double* log_score, double* marginal, double* log_partition, double* scale, void* stream)
{
    if (L < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: L must be >= 0%s");
    if (S < 1 || S > horizon::MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: S must lie in 1 .. 2048 (the states live in LDS)%s");
    if (!(dz > 0.0) || !std::isfinite(dz)) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: dz must be positive and finite%s");
    if (!(switch_cost >= 0.0) || !std::isfinite(switch_cost)) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: switch must be >= 0 and finite%s");
    if (L == 0) return GBP_OK;
    if (total_n < L || max_n < 1 || max_n > total_n || total_n > (int64_t)max_n * L)
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: total_n and max_n do not fit L sequences of at least one sounding%s");
    if (total_n > 0x7fffffffffffffffLL / 8 / (S + 1))
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: total_n * (S + 1) out of range%s");
    if (!ptr) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: ptr is NULL%s");
    if (!score || !g || !d) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: NULL pointer (score, g, d)%s");
    if (!back) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: the back workspace is NULL%s");
    if (!cell || !log_score) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: NULL pointer (cell, log_score)%s");
    if ((marginal != nullptr) != (log_partition != nullptr) || (marginal != nullptr) != (scale != nullptr))
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_track: marginal, log_partition and scale go together (all, or all NULL)%s");
    hipStream_t st = (hipStream_t)stream;
#define GBP_HORIZON_CASE(nj) \
    case nj: return horizon_launch<nj>(L, ptr, S, dz, score, absent_score, g, d, switch_cost, back, cell, log_score, marginal, log_partition, scale, st)
    switch ((S + 1 + horizon::THREADS - 1) / horizon::THREADS) {
        GBP_HORIZON_CASE(1);
        GBP_HORIZON_CASE(2);
        GBP_HORIZON_CASE(3);
        GBP_HORIZON_CASE(4);
        GBP_HORIZON_CASE(5);
        GBP_HORIZON_CASE(6);
        GBP_HORIZON_CASE(7);
        GBP_HORIZON_CASE(8);
        default: return horizon_launch<horizon::MAX_OWNED>(L, ptr, S, dz, score, absent_score, g, d, switch_cost, back, cell, log_score, marginal,
                                                           log_partition, scale, st);
    }
#undef GBP_HORIZON_CASE
}

#include "gbp_horizon_unit.h"

// Horizon pairs (gbp_horizon_unit.h): one workgroup per sequence walks the chain over the ordered pairs of cells; the Viterbi launch
// always, the forward-backward launch only when the marginals are asked for.  Every refusal comes before any launch; ptr is not read
// on the host.
extern "C" gbp_status gbp_horizon_unit_track(int L, const int64_t* ptr, int64_t total_n, int max_n, int S, int min_cells, double dz,
                                             const double* score_top, const double* score_base, const double* thickness_score,
                                             const double* absent_score, const double* g, const double* d, double switch_cost, uint8_t* back,
                                             int32_t* back_absent, int32_t* cell_top, int32_t* cell_base, double* log_score, double* alpha,
                                             double* marginal_top, double* marginal_base, double* marginal_thickness, double* marginal_absent,
                                             double* log_partition, double* scale, void* stream)
{
    if (L < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: L must be >= 0%s");
    if (S < 1 || S > horizon_unit::MAX_UNIT_STATES) {
        char most[16];
        std::snprintf(most, sizeof(most), "%d", horizon_unit::MAX_UNIT_STATES);
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: S must lie in 1 .. %s (two S x S matrices live in LDS)", most);
    }
    if (min_cells < 0 || min_cells > S - 1) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: min_cells must lie in 0 .. S - 1%s");
    if (!(dz > 0.0) || !std::isfinite(dz)) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: dz must be positive and finite%s");
    if (!(switch_cost >= 0.0) || !std::isfinite(switch_cost))
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: switch must be >= 0 and finite%s");
    if (L == 0) return GBP_OK;
    if (total_n < L || max_n < 1 || max_n > total_n || total_n > (int64_t)max_n * L)
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: total_n and max_n do not fit L sequences of at least one sounding%s");
    if (total_n > 0x7fffffffffffffffLL / 8 / ((int64_t)S * S + 1))
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: total_n * (S * S + 1) out of range%s");
    if (!ptr) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: ptr is NULL%s");
    if (!score_top || !score_base || !g || !d) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: NULL pointer (score_top, score_base, g, d)%s");
    if (!back || (absent_score && !back_absent)) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: a back workspace is NULL%s");
    if (!cell_top || !cell_base || !log_score) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: NULL pointer (cell_top, cell_base, log_score)%s");
    const int given = (alpha != nullptr) + (marginal_top != nullptr) + (marginal_base != nullptr) + (marginal_thickness != nullptr) +
                      (marginal_absent != nullptr) + (log_partition != nullptr) + (scale != nullptr);
    if (given != 0 && given != 7)
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_unit_track: alpha, the four marginals, log_partition and scale go together (all, or all NULL)%s");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = horizon_unit::lds_doubles(S) * sizeof(double);
    const int has_absent = absent_score ? 1 : 0, has_ts = thickness_score ? 1 : 0;
    if (lds > 48 * 1024) {                                                  // (above the default limit of a launch's dynamic LDS)
        (void)hipFuncSetAttribute((const void*)horizon_unit::k_unit_viterbi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void*)horizon_unit::k_unit_marginals, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    unsigned char* back1 = (unsigned char*)back;
    hipLaunchKernelGGL(horizon_unit::k_unit_viterbi, dim3((unsigned)L), dim3(horizon_unit::THREADS), lds, st, (const long long*)ptr, S, min_cells,
                       has_absent, has_ts, dz, score_top, score_base, thickness_score, absent_score, g, d, switch_cost, back1,
                       back1 + (size_t)total_n * S * S, (int*)back_absent, (int*)cell_top, (int*)cell_base, log_score);
    GBP_HIP(hipGetLastError());
    if (given) {
        hipLaunchKernelGGL(horizon_unit::k_unit_marginals, dim3((unsigned)L), dim3(horizon_unit::THREADS), lds, st, (const long long*)ptr, S,
                           min_cells, has_absent, has_ts, dz, score_top, score_base, thickness_score, absent_score, g, d, switch_cost, alpha,
                           marginal_top, marginal_base, marginal_thickness, marginal_absent, log_partition, scale);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

#include "gbp_section.h"

// Sections of sampled models (gbp_section.h): one workgroup per sequence walks the chain over the kept models; the Viterbi launch
// always, the forward-backward launch only when the marginals are asked for.  Every refusal comes before any launch; ptr is not read
// on the host.
namespace {

template <int NJ>
gbp_status section_launch(int L, const int64_t* ptr, int n, const int32_t* n_used, const double* score, const double* g, const double* d2,
                          uint16_t* back, int32_t* state, double* log_score, double* marginal, double* log_partition, double* scale,
                          hipStream_t st)
{
    const size_t lds = section::lds_bytes(n);
    const int W = n <= 64 ? 64 : n <= 128 ? 128 : section::THREADS;        // lanes that own a state; the other lane groups share the i range
    hipLaunchKernelGGL(section::k_section_viterbi<NJ>, dim3((unsigned)L), dim3(section::THREADS), lds, st, (const long long*)ptr, n, W,
                       (const int*)n_used, score, g, d2, (unsigned short*)back, (int*)state, log_score);
    GBP_HIP(hipGetLastError());
    if (marginal) {
        hipLaunchKernelGGL(section::k_section_marginals<NJ>, dim3((unsigned)L), dim3(section::THREADS), lds, st, (const long long*)ptr, n,
                           (const int*)n_used, score, g, d2, marginal, log_partition, scale);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

}  // namespace

extern "C" gbp_status gbp_section_track(int L, const int64_t* ptr, int64_t total_n, int n, const int32_t* n_used, const double* score,
                                        const double* g, const double* d2, uint16_t* back, int32_t* state, double* log_score,
                                        double* marginal, double* log_partition, double* scale, void* stream)
{
    if (L < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: L must be >= 0%s");
    if (n < 1 || n > section::MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: n must lie in 1 .. 1024%s");
    if (L == 0) return GBP_OK;
    if (total_n < L) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: total_n does not fit L sequences of at least one sounding%s");
    if (total_n > 0x7fffffffffffffffLL / 8 / n / n) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: total_n * n * n out of range%s");
    if (!ptr) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: ptr is NULL%s");
    if (!n_used || !score || !g || !d2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: NULL pointer (n_used, score, g, d2)%s");
    if (!back) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: the back workspace is NULL%s");
    if (!state || !log_score) return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: NULL pointer (state, log_score)%s");
    if ((marginal != nullptr) != (log_partition != nullptr) || (marginal != nullptr) != (scale != nullptr))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_track: marginal, log_partition and scale go together (all, or all NULL)%s");
    hipStream_t st = (hipStream_t)stream;
    switch ((n + section::THREADS - 1) / section::THREADS) {
        case 1: return section_launch<1>(L, ptr, n, n_used, score, g, d2, back, state, log_score, marginal, log_partition, scale, st);
        case 2: return section_launch<2>(L, ptr, n, n_used, score, g, d2, back, state, log_score, marginal, log_partition, scale, st);
        case 3: return section_launch<3>(L, ptr, n, n_used, score, g, d2, back, state, log_score, marginal, log_partition, scale, st);
        default: return section_launch<section::MAX_OWNED>(L, ptr, n, n_used, score, g, d2, back, state, log_score, marginal, log_partition,
                                                           scale, st);
    }
}

// Joint draws of sections (gbp_section.h k_section_filter, k_section_draw): the filter launch, one workgroup per sequence, then the
// walks, one wave per (sequence, 64 realisations).  Every refusal comes before any launch; ptr is not read on the host.
namespace {

template <int NJ>
gbp_status section_draw_launch(int L, const int64_t* ptr, int64_t total_n, int n, const int32_t* n_used, const double* score, const double* g,
                               const double* d2, const int64_t* row_key, uint64_t seed, int n_draws, double* filtered, double* scale,
                               int32_t* draw_state, hipStream_t st)
{
    hipLaunchKernelGGL(section::k_section_filter<NJ>, dim3((unsigned)L), dim3(section::THREADS), section::lds_bytes(n), st, (const long long*)ptr, n,
                       (const int*)n_used, score, g, d2, filtered, scale);
    GBP_HIP(hipGetLastError());
    hipLaunchKernelGGL(section::k_section_draw, dim3((unsigned)L, (unsigned)((n_draws + 63) / 64)), dim3(64), 0, st, (const long long*)ptr,
                       (long long)total_n, n, (const int*)n_used, g, d2, (const long long*)row_key, (unsigned long long)seed, n_draws,
                       (const double*)filtered, (int*)draw_state);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

}  // namespace

extern "C" gbp_status gbp_section_draw(int L, const int64_t* ptr, int64_t total_n, int n, const int32_t* n_used, const double* score,
                                       const double* g, const double* d2, const int64_t* row_key, uint64_t seed, int n_draws,
                                       double* filtered, double* scale, int32_t* draw_state, void* stream)
{
    if (L < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: L must be >= 0%s");
    if (n < 1 || n > section::MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: n must lie in 1 .. 1024%s");
    if (n_draws < 1 || n_draws > section::MAX_DRAWS) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: n_draws must lie in 1 .. 65536%s");
    if (L == 0) return GBP_OK;
    if (total_n < L) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: total_n does not fit L sequences of at least one sounding%s");
    if (total_n > 0x7fffffffffffffffLL / 8 / n / n) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: total_n * n * n out of range%s");
    if (total_n > 0x7fffffffffffffffLL / 4 / n_draws) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: n_draws * total_n out of range%s");
    if (!ptr) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: ptr is NULL%s");
    if (!n_used || !score || !g || !d2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: NULL pointer (n_used, score, g, d2)%s");
    if (!filtered || !scale) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: NULL pointer (filtered, the scale workspace)%s");
    if (!draw_state) return fail(GBP_ERR_INVALID_ARG, "gbp_section_draw: draw_state is NULL%s");
    hipStream_t st = (hipStream_t)stream;
    switch ((n + section::THREADS - 1) / section::THREADS) {
        case 1: return section_draw_launch<1>(L, ptr, total_n, n, n_used, score, g, d2, row_key, seed, n_draws, filtered, scale, draw_state, st);
        case 2: return section_draw_launch<2>(L, ptr, total_n, n, n_used, score, g, d2, row_key, seed, n_draws, filtered, scale, draw_state, st);
        case 3: return section_draw_launch<3>(L, ptr, total_n, n, n_used, score, g, d2, row_key, seed, n_draws, filtered, scale, draw_state, st);
        default: return section_draw_launch<section::MAX_OWNED>(L, ptr, total_n, n, n_used, score, g, d2, row_key, seed, n_draws, filtered, scale,
                                                                draw_state, st);
    }
}

#include "gbp_section_evidence.h"

// The evidence of the lateral coupling (gbp_section_evidence.h): one launch, one workgroup per sequence, an instance per (columns a
// thread owns, rungs).  Every refusal comes before any launch; ptr is not read on the host.
namespace {

template <int NJ, int T>
gbp_status section_evidence_launch(int L, const int64_t* ptr, int n, const int32_t* n_used, const double* score, const double* g,
                                   const double* d2, double* log_partition, double* dlog_partition, hipStream_t st)
{
    const size_t lds = section::evidence_lds_bytes(n, T);
    if (lds > 48 * 1024) {                                                  // (above the default limit of a launch's dynamic LDS)
        (void)hipFuncSetAttribute((const void*)section::k_section_evidence<NJ, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL((section::k_section_evidence<NJ, T>), dim3((unsigned)L), dim3(section::THREADS), lds, st, (const long long*)ptr, L, n,
                       section::evidence_width(n), (const int*)n_used, score, g, d2, log_partition, dlog_partition);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

}  // namespace

extern "C" gbp_status gbp_section_evidence(int L, const int64_t* ptr, int64_t total_n, int n, const int32_t* n_used, const double* score,
                                           const double* g, const double* d2, int T, double* log_partition, double* dlog_partition,
                                           void* stream)
{
    if (L < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: L must be >= 0%s");
    if (n < 1 || n > section::MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: n must lie in 1 .. 1024%s");
    if (T < 1 || T > section::EVIDENCE_MAX_RUNGS) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: T must lie in 1 .. 8%s");
    if (T * n > section::EVIDENCE_MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: T * n must not exceed 2048%s");
    if (L == 0) return GBP_OK;
    if (total_n < L) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: total_n does not fit L sequences of at least one sounding%s");
    if (total_n > 0x7fffffffffffffffLL / 8 / n / n) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: total_n * n * n out of range%s");
    if (!ptr) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: ptr is NULL%s");
    if (!n_used || !score || !g || !d2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: NULL pointer (n_used, score, g, d2)%s");
    if (!log_partition || !dlog_partition)
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: NULL pointer (log_partition, dlog_partition)%s");
    hipStream_t st = (hipStream_t)stream;
#define GBP_EVIDENCE_CASE(NJ_, T_)                                                                                                         \
    case (NJ_) * 16 + (T_): return section_evidence_launch<NJ_, T_>(L, ptr, n, n_used, score, g, d2, log_partition, dlog_partition, st)
    switch ((n + section::THREADS - 1) / section::THREADS * 16 + T) {       // T * n <= 2048 leaves these twenty
        GBP_EVIDENCE_CASE(1, 1); GBP_EVIDENCE_CASE(1, 2); GBP_EVIDENCE_CASE(1, 3); GBP_EVIDENCE_CASE(1, 4);
        GBP_EVIDENCE_CASE(1, 5); GBP_EVIDENCE_CASE(1, 6); GBP_EVIDENCE_CASE(1, 7); GBP_EVIDENCE_CASE(1, 8);
        GBP_EVIDENCE_CASE(2, 1); GBP_EVIDENCE_CASE(2, 2); GBP_EVIDENCE_CASE(2, 3); GBP_EVIDENCE_CASE(2, 4);
        GBP_EVIDENCE_CASE(2, 5); GBP_EVIDENCE_CASE(2, 6); GBP_EVIDENCE_CASE(2, 7);
        GBP_EVIDENCE_CASE(3, 1); GBP_EVIDENCE_CASE(3, 2); GBP_EVIDENCE_CASE(3, 3);
        GBP_EVIDENCE_CASE(4, 1); GBP_EVIDENCE_CASE(4, 2);
        default: return fail(GBP_ERR_INVALID_ARG, "gbp_section_evidence: T * n must not exceed 2048%s");
    }
#undef GBP_EVIDENCE_CASE
}

#include "gbp_section_graph.h"

// Sections across lines (gbp_section_graph.h): K and the first messages, one launch per sweep with one workgroup per undirected edge,
// the residuals of all sweeps in one launch, the beliefs.  Every refusal comes before any launch; no device array is read on the host.
extern "C" gbp_status gbp_section_propagate(int S, int E, int n, const int32_t* eu, const int32_t* ev, const int32_t* n_used,
                                            const double* score, const double* g, const double* d2, const int32_t* in_ptr,
                                            const int32_t* in_edge, int sweeps, double damping, double* K, double* w, double* mu,
                                            double* resid, double* belief, int32_t* state, double* residual, void* stream)
{
    if (S < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: S must be >= 0%s");
    if (E < 0 || E > 0x3fffffff) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: E must lie in 0 .. 2^30 - 1%s");
    if (n < 1 || n > section::GRAPH_MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: n must lie in 1 .. 256%s");
    if (sweeps < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: sweeps must be >= 1%s");
    if (!(damping >= 0.0 && damping < 1.0)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: damping must lie in [0, 1)%s");
    if (E > 0 && S < 2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: an edge needs two soundings%s");
    if ((long long)S + 2LL * E > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: S + 2 E out of range%s");
    if (E > 0 && (long long)E > 0x7fffffffffffffffLL / 8 / n / n) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: E * n * n out of range%s");
    if (E > 0 && (long long)sweeps > 0x7fffffffffffffffLL / 16 / E) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: sweeps * 2 E out of range%s");
    if (!residual) return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: residual is NULL%s");
    if (S > 0 && (!n_used || !score || !in_ptr || !w || !belief || !state))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: NULL pointer (n_used, score, in_ptr, w, belief, state)%s");
    if (E > 0 && (!eu || !ev || !g || !d2 || !in_edge || !K || !mu || !resid))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_propagate: NULL pointer (eu, ev, g, d2, in_edge, K, mu, resid)%s");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(section::THREADS);
    const size_t half = (size_t)2 * E * n;                                  // one message buffer
    if (E > 0) {
        hipLaunchKernelGGL(section::k_graph_kernel, dim3((unsigned)E), block, 0, st, S, n, (const int*)eu, (const int*)ev, (const int*)n_used, g, d2, K);
        GBP_HIP(hipGetLastError());
    }
    if (S > 0) {
        hipLaunchKernelGGL(section::k_graph_init, dim3((unsigned)(S + 2 * E)), block, 0, st, S, E, n, (const int*)eu, (const int*)ev,
                           (const int*)n_used, score, w, mu, mu ? mu + half : mu);
        GBP_HIP(hipGetLastError());
    }
    for (int t = 0; E > 0 && t < sweeps; ++t) {
        const double* from = mu + (size_t)(t & 1) * half;
        double* to = mu + (size_t)((t + 1) & 1) * half;
        double* r = resid + (size_t)t * 2 * E;
#define GBP_GRAPH_SWEEP(DAMP, MAXN)                                                                                                      \
    hipLaunchKernelGGL((section::k_graph_sweep<DAMP, MAXN>), dim3((unsigned)E), block, 0, st, S, E, n, (const int*)eu, (const int*)ev,     \
                       (const int*)n_used, (const double*)w, (const double*)K, (const int*)in_ptr, (const int*)in_edge, from, to, damping, r)
        if (n <= 64) {
            if (damping != 0.0) GBP_GRAPH_SWEEP(true, 64);
            else GBP_GRAPH_SWEEP(false, 64);
        } else {
            if (damping != 0.0) GBP_GRAPH_SWEEP(true, section::GRAPH_MAX_STATES);
            else GBP_GRAPH_SWEEP(false, section::GRAPH_MAX_STATES);
        }
#undef GBP_GRAPH_SWEEP
        GBP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(section::k_graph_residual, dim3((unsigned)sweeps), block, 0, st, 2LL * E, (const double*)resid, residual);
    GBP_HIP(hipGetLastError());
    if (S > 0) {
        hipLaunchKernelGGL(section::k_graph_belief, dim3((unsigned)S), block, 0, st, E, n, (const int*)n_used, (const double*)w, (const int*)in_ptr,
                           (const int*)in_edge, (const double*)(mu ? mu + (size_t)(sweeps & 1) * half : mu), belief, (int*)state);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

// The terms of the Bethe evidence (gbp_section_evidence.h k_graph_evidence): one launch, a workgroup per edge and one per sounding.
extern "C" gbp_status gbp_section_graph_evidence(int S, int E, int n, const int32_t* eu, const int32_t* ev, const int32_t* n_used,
                                                 const double* w, const double* g, const double* d2, const int32_t* in_ptr,
                                                 const int32_t* in_edge, const double* message, double* node_log_z, double* edge_log_z,
                                                 double* edge_energy, void* stream)
{
    if (S < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: S must be >= 0%s");
    if (E < 0 || E > 0x3fffffff) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: E must lie in 0 .. 2^30 - 1%s");
    if (n < 1 || n > section::GRAPH_MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: n must lie in 1 .. 256%s");
    if (E > 0 && S < 2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: an edge needs two soundings%s");
    if ((long long)S + 2LL * E > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: S + 2 E out of range%s");
    if (E > 0 && (long long)E > 0x7fffffffffffffffLL / 8 / n / n)
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: E * n * n out of range%s");
    if (S > 0 && (!n_used || !w || !in_ptr || !node_log_z))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: NULL pointer (n_used, w, in_ptr, node_log_z)%s");
    if (E > 0 && (!eu || !ev || !g || !d2 || !in_edge || !message || !edge_log_z || !edge_energy))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_evidence: NULL pointer (eu, ev, g, d2, in_edge, message, edge_log_z, edge_energy)%s");
    if (S == 0) return GBP_OK;
    hipLaunchKernelGGL(section::k_graph_evidence, dim3((unsigned)(E + S)), dim3(section::THREADS), 0, (hipStream_t)stream, S, E, n, (const int*)eu,
                       (const int*)ev, (const int*)n_used, w, g, d2, (const int*)in_ptr, (const int*)in_edge, message, node_log_z, edge_log_z,
                       edge_energy);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

#include "gbp_section_graph_path.h"

// level_ptr / colour_ptr (HOST, [count + 1]): from 0 to S without a decrease.
static bool graph_groups_fit(const int32_t* group_ptr, int count, int S)
{
    if (group_ptr[0] != 0 || group_ptr[count] != S) return false;
    for (int c = 0; c < count; ++c)
        if (group_ptr[c + 1] < group_ptr[c]) return false;
    return true;
}

// The most probable section (gbp_section_graph_path.h): the messages start at 0.0, one launch per sweep with one workgroup per undirected
// edge, the residuals of all sweeps in one launch, the max-marginals, then the decode with one launch per breadth-first level.  Every
// refusal comes before any launch; no device array is read on the host (level_ptr is a host array).
extern "C" gbp_status gbp_section_graph_path(int S, int E, int n, const int32_t* eu, const int32_t* ev, const int32_t* n_used,
                                             const double* score, const double* g, const double* d2, const int32_t* in_ptr,
                                             const int32_t* in_edge, int sweeps, double damping, int n_levels, const int32_t* level_ptr,
                                             const int32_t* level_node, const int32_t* level, double* nu, double* resid,
                                             double* max_marginal, int32_t* decoded_state, double* residual, void* stream)
{
    if (S < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: S must be >= 0%s");
    if (E < 0 || E > 0x3fffffff) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: E must lie in 0 .. 2^30 - 1%s");
    if (n < 1 || n > section::GRAPH_MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: n must lie in 1 .. 256%s");
    if (sweeps < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: sweeps must be >= 1%s");
    if (!(damping >= 0.0 && damping < 1.0)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: damping must lie in [0, 1)%s");
    if (E > 0 && S < 2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: an edge needs two soundings%s");
    if ((long long)S + 2LL * E > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: S + 2 E out of range%s");
    if (E > 0 && (long long)E > 0x7fffffffffffffffLL / 8 / n / n) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: E * n * n out of range%s");
    if (E > 0 && (long long)sweeps > 0x7fffffffffffffffLL / 16 / E) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: sweeps * 2 E out of range%s");
    if (S > 0 && (n_levels < 1 || n_levels > S)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: n_levels must lie in 1 .. S%s");
    if (S > 0 && (!n_used || !score || !in_ptr || !level_ptr || !level_node || !level))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: NULL pointer (n_used, score, in_ptr, level_ptr, level_node, level)%s");
    if (S > 0 && (!max_marginal || !decoded_state || !residual))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: NULL pointer (max_marginal, decoded_state, residual)%s");
    if (E > 0 && (!eu || !ev || !g || !d2 || !in_edge || !nu || !resid))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: NULL pointer (eu, ev, g, d2, in_edge, nu, resid)%s");
    if (S == 0) return GBP_OK;
    if (!graph_groups_fit(level_ptr, n_levels, S))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_path: level_ptr must start at 0, not decrease and end at S%s");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(section::THREADS);
    const size_t half = (size_t)2 * E * n;                                  // one message buffer
    if (E > 0) GBP_HIP(hipMemsetAsync(nu, 0, 2 * half * sizeof(double), st));
    for (int t = 0; E > 0 && t < sweeps; ++t) {
        const double* from = nu + (size_t)(t & 1) * half;
        double* to = nu + (size_t)((t + 1) & 1) * half;
        double* r = resid + (size_t)t * 2 * E;
#define GBP_GRAPH_MAXSUM(DAMP, MAXN)                                                                                                     \
    hipLaunchKernelGGL((section::k_graph_maxsum<DAMP, MAXN>), dim3((unsigned)E), block, 0, st, S, E, n, (const int*)eu, (const int*)ev,    \
                       (const int*)n_used, score, g, d2, (const int*)in_ptr, (const int*)in_edge, from, to, damping, r)
        if (n <= 64) {
            if (damping != 0.0) GBP_GRAPH_MAXSUM(true, 64);
            else GBP_GRAPH_MAXSUM(false, 64);
        } else {
            if (damping != 0.0) GBP_GRAPH_MAXSUM(true, section::GRAPH_MAX_STATES);
            else GBP_GRAPH_MAXSUM(false, section::GRAPH_MAX_STATES);
        }
#undef GBP_GRAPH_MAXSUM
        GBP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(section::k_graph_residual, dim3((unsigned)sweeps), block, 0, st, 2LL * E, (const double*)resid, residual);
    GBP_HIP(hipGetLastError());
    const double* last = nu ? nu + (size_t)(sweeps & 1) * half : nu;
    hipLaunchKernelGGL(section::k_graph_maxmarginal, dim3((unsigned)S), block, 0, st, E, n, (const int*)n_used, score, (const int*)in_ptr,
                       (const int*)in_edge, last, max_marginal);
    GBP_HIP(hipGetLastError());
    for (int l = 0; l < n_levels; ++l) {
        const int count = level_ptr[l + 1] - level_ptr[l];
        if (count == 0) continue;
        hipLaunchKernelGGL(section::k_graph_condition<false>, dim3((unsigned)count), block, 0, st, S, E, n, (const int*)eu, (const int*)ev,
                           (const int*)n_used, score, g, d2, (const int*)in_ptr, (const int*)in_edge, last, (const int*)level,
                           (const int*)level_node + level_ptr[l], count, (int*)decoded_state, (int*)nullptr, 0);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

// Coordinate ascent on the exact score (gbp_section_graph_path.h k_graph_condition<true>): per sweep one launch per colour of soundings,
// a workgroup for every (candidate, sounding of the colour).  All `refine` sweeps are launched: a candidate that has stopped moving
// adds nothing to its later counters, and no counter is read on the host.  Every refusal comes before any launch.
extern "C" gbp_status gbp_section_graph_refine(int S, int E, int n, int C, const int32_t* eu, const int32_t* ev, const int32_t* n_used,
                                               const double* score, const double* g, const double* d2, const int32_t* in_ptr,
                                               const int32_t* in_edge, int n_colours, const int32_t* colour_ptr,
                                               const int32_t* colour_node, int refine, int32_t* state, int32_t* moves, void* stream)
{
    if (S < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: S must be >= 0%s");
    if (E < 0 || E > 0x3fffffff) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: E must lie in 0 .. 2^30 - 1%s");
    if (n < 1 || n > section::GRAPH_MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: n must lie in 1 .. 256%s");
    if (C < 1 || C > section::MAX_DRAWS + 1) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: C must lie in 1 .. 65537%s");
    if (refine < 0 || refine > 65536) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: refine must lie in 0 .. 65536%s");
    if (E > 0 && S < 2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: an edge needs two soundings%s");
    if ((long long)S + 2LL * E > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: S + 2 E out of range%s");
    if (E > 0 && (long long)E > 0x7fffffffffffffffLL / 8 / n / n) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: E * n * n out of range%s");
    if ((long long)C * S > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: C * S out of range%s");
    if (S > 0 && (n_colours < 1 || n_colours > S)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: n_colours must lie in 1 .. S%s");
    if (S > 0 && (!n_used || !score || !in_ptr || !colour_ptr || !colour_node || !state))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: NULL pointer (n_used, score, in_ptr, colour_ptr, colour_node, state)%s");
    if (S > 0 && refine > 0 && !moves) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: moves is NULL%s");
    if (E > 0 && (!eu || !ev || !g || !d2 || !in_edge)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: NULL pointer (eu, ev, g, d2, in_edge)%s");
    if (S == 0 || refine == 0) return GBP_OK;
    if (!graph_groups_fit(colour_ptr, n_colours, S))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_refine: colour_ptr must start at 0, not decrease and end at S%s");
    hipStream_t st = (hipStream_t)stream;
    GBP_HIP(hipMemsetAsync(moves, 0, (size_t)C * refine * sizeof(int32_t), st));
    for (int t = 0; t < refine; ++t) {
        for (int c = 0; c < n_colours; ++c) {
            const int count = colour_ptr[c + 1] - colour_ptr[c];
            if (count == 0) continue;
            hipLaunchKernelGGL(section::k_graph_condition<true>, dim3((unsigned)((long long)C * count)), dim3(section::THREADS), 0, st, S, E, n,
                               (const int*)eu, (const int*)ev, (const int*)n_used, score, g, d2, (const int*)in_ptr, (const int*)in_edge,
                               (const double*)nullptr, (const int*)nullptr, (const int*)colour_node + colour_ptr[c], count, (int*)state,
                               (int*)moves + t, refine);
            GBP_HIP(hipGetLastError());
        }
    }
    return GBP_OK;
}

#include "gbp_horizon_graph.h"

// Horizons across lines (gbp_horizon_graph.h): the sweeps of both semirings, one launch each with one workgroup per undirected edge.
namespace {

template <bool SUM, int NJ, bool SPLIT>
gbp_status hgraph_sweep_launch(int N, int E, int S, int has_absent, double dz, double sw, const int32_t* eu, const int32_t* ev,
                               const double* node, const double* g, const double* d, const int32_t* in_ptr, const int32_t* in_edge,
                               const double* from, double* to, double damping, double* resid, hipStream_t st)
{
    const size_t lds = horizon_graph::sweep_lds_bytes(S);
    if (lds > 48 * 1024) {                                                  // (above the default limit of a launch's dynamic LDS)
        (void)hipFuncSetAttribute((const void*)horizon_graph::k_hgraph_sweep<SUM, false, NJ, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipFuncSetAttribute((const void*)horizon_graph::k_hgraph_sweep<SUM, true, NJ, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    if (damping != 0.0)
        hipLaunchKernelGGL((horizon_graph::k_hgraph_sweep<SUM, true, NJ, SPLIT>), dim3((unsigned)E), dim3(horizon_graph::THREADS), lds, st, N, E, S,
                           has_absent, dz, sw, (const int*)eu, (const int*)ev, node, g, d, (const int*)in_ptr, (const int*)in_edge, from, to, damping,
                           resid);
    else
        hipLaunchKernelGGL((horizon_graph::k_hgraph_sweep<SUM, false, NJ, SPLIT>), dim3((unsigned)E), dim3(horizon_graph::THREADS), lds, st, N, E, S,
                           has_absent, dz, sw, (const int*)eu, (const int*)ev, node, g, d, (const int*)in_ptr, (const int*)in_edge, from, to, damping,
                           resid);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

// Sweep t = 0 .. sweeps - 1 reads half t & 1 of msg [2, 2 E, SA] and writes the other one; resid [sweeps, 2 E].
template <bool SUM>
gbp_status hgraph_sweeps(int N, int E, int S, int has_absent, double dz, double sw, const int32_t* eu, const int32_t* ev, const double* node,
                         const double* g, const double* d, const int32_t* in_ptr, const int32_t* in_edge, int sweeps, double damping,
                         double* msg, double* resid, hipStream_t st)
{
    const int SA = S + has_absent;
    const size_t half = (size_t)2 * E * SA;
    for (int t = 0; t < sweeps; ++t) {
        const double* from = msg + (size_t)(t & 1) * half;
        double* to = msg + (size_t)((t + 1) & 1) * half;
        double* r = resid + (size_t)t * 2 * E;
        gbp_status rc;
#define GBP_HGRAPH_CASE(nj) \
    case nj: rc = hgraph_sweep_launch<SUM, nj, false>(N, E, S, has_absent, dz, sw, eu, ev, node, g, d, in_ptr, in_edge, from, to, damping, r, st); break
        if (SA <= horizon_graph::SPLIT_STATES) {
            rc = hgraph_sweep_launch<SUM, 1, true>(N, E, S, has_absent, dz, sw, eu, ev, node, g, d, in_ptr, in_edge, from, to, damping, r, st);
        } else {
            switch ((SA + horizon_graph::THREADS - 1) / horizon_graph::THREADS) {
                GBP_HGRAPH_CASE(1);
                GBP_HGRAPH_CASE(2);
                GBP_HGRAPH_CASE(3);
                GBP_HGRAPH_CASE(4);
                GBP_HGRAPH_CASE(5);
                GBP_HGRAPH_CASE(6);
                GBP_HGRAPH_CASE(7);
                GBP_HGRAPH_CASE(8);
                default:
                    rc = hgraph_sweep_launch<SUM, horizon_graph::MAX_OWNED, false>(N, E, S, has_absent, dz, sw, eu, ev, node, g, d, in_ptr, in_edge, from,
                                                                                   to, damping, r, st);
            }
        }
#undef GBP_HGRAPH_CASE
        if (rc != GBP_OK) return rc;
    }
    return GBP_OK;
}

// The refusals the three entries share, without the entry's name (hgraph_fail puts it in front); NULL when the arguments fit.
const char* hgraph_refusal(int N, int E, int S, int has_absent, double dz, double sw)
{
    if (N < 0) return "N must be >= 0";
    if (E < 0 || E > 0x3fffffff) return "E must lie in 0 .. 2^30 - 1";
    if (S < 1 || S > horizon_graph::MAX_STATES) return "S must lie in 1 .. 2048 (the states live in LDS)";
    if (has_absent != 0 && has_absent != 1) return "has_absent must be 0 or 1";
    if (!(dz > 0.0) || !std::isfinite(dz)) return "dz must be positive and finite";
    if (!(sw >= 0.0) || !std::isfinite(sw)) return "switch must be >= 0 and finite";
    if (E > 0 && N < 2) return "an edge needs two soundings";
    if ((long long)N + 2LL * E > 0x7fffffffLL) return "N + 2 E out of range";
    return nullptr;
}

gbp_status hgraph_fail(const char* entry, const char* why)
{
    char text[256];
    std::snprintf(text, sizeof text, "%s: %s", entry, why);
    return fail(GBP_ERR_INVALID_ARG, "%s", text);
}

}  // namespace

// Beliefs of a horizon on the survey graph: w and the first messages, one launch per sweep, the residuals of all sweeps in one launch,
// the beliefs.  Every refusal comes before any launch; no device array is read on the host.
extern "C" gbp_status gbp_horizon_graph_propagate(int N, int E, int S, int has_absent, double dz, double switch_cost, const int32_t* eu,
                                                  const int32_t* ev, const double* score, const double* g, const double* d,
                                                  const int32_t* in_ptr, const int32_t* in_edge, int sweeps, double damping, double* w,
                                                  double* mu, double* resid, double* belief, int32_t* state, double* residual, void* stream)
{
    static const char* const entry = "gbp_horizon_graph_propagate";
    if (const char* why = hgraph_refusal(N, E, S, has_absent, dz, switch_cost)) return hgraph_fail(entry, why);
    const int SA = S + has_absent;
    if (sweeps < 1) return hgraph_fail(entry, "sweeps must be >= 1");
    if (!(damping >= 0.0 && damping < 1.0)) return hgraph_fail(entry, "damping must lie in [0, 1)");
    if ((long long)N > 0x7fffffffffffffffLL / 8 / SA) return hgraph_fail(entry, "N * SA out of range");
    if ((long long)E > 0x7fffffffffffffffLL / 32 / SA) return hgraph_fail(entry, "2 * 2 E * SA out of range");
    if (E > 0 && (long long)sweeps > 0x7fffffffffffffffLL / 16 / E) return hgraph_fail(entry, "sweeps * 2 E out of range");
    if (!residual) return hgraph_fail(entry, "residual is NULL");
    if (N > 0 && (!score || !in_ptr || !w || !belief || !state)) return hgraph_fail(entry, "NULL pointer (score, in_ptr, w, belief, state)");
    if (E > 0 && (!eu || !ev || !g || !d || !in_edge || !mu || !resid))
        return hgraph_fail(entry, "NULL pointer (eu, ev, g, d, in_edge, mu, resid)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(horizon_graph::THREADS);
    const size_t half = (size_t)2 * E * SA;
    if (N > 0) {
        hipLaunchKernelGGL(horizon_graph::k_hgraph_init, dim3((unsigned)(N + 2 * E)), block, 0, st, N, SA, score, w, mu, mu ? mu + half : mu);
        GBP_HIP(hipGetLastError());
    }
    if (E > 0) {
        const gbp_status rc = hgraph_sweeps<true>(N, E, S, has_absent, dz, switch_cost, eu, ev, w, g, d, in_ptr, in_edge, sweeps, damping, mu, resid, st);
        if (rc != GBP_OK) return rc;
    }
    hipLaunchKernelGGL(section::k_graph_residual, dim3((unsigned)sweeps), block, 0, st, 2LL * E, (const double*)resid, residual);
    GBP_HIP(hipGetLastError());
    if (N > 0) {
        hipLaunchKernelGGL(horizon_graph::k_hgraph_node<true>, dim3((unsigned)N), block, 0, st, E, SA, (const double*)w, (const int*)in_ptr,
                           (const int*)in_edge, (const double*)(mu ? mu + (size_t)(sweeps & 1) * half : mu), belief, (int*)state);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

// The most probable horizon: the messages start at 0.0, one launch per sweep, the residuals, the max-marginals, then the decode with one
// launch per breadth-first level.  Every refusal comes before any launch; level_ptr is a host array, no device array is read on the host.
extern "C" gbp_status gbp_horizon_graph_path(int N, int E, int S, int has_absent, double dz, double switch_cost, const int32_t* eu,
                                             const int32_t* ev, const double* score, const double* g, const double* d,
                                             const int32_t* in_ptr, const int32_t* in_edge, int sweeps, double damping, int n_levels,
                                             const int32_t* level_ptr, const int32_t* level_node, const int32_t* level, double* nu,
                                             double* resid, double* max_marginal, int32_t* decoded_state, double* residual, void* stream)
{
    static const char* const entry = "gbp_horizon_graph_path";
    if (const char* why = hgraph_refusal(N, E, S, has_absent, dz, switch_cost)) return hgraph_fail(entry, why);
    const int SA = S + has_absent;
    if (sweeps < 1) return hgraph_fail(entry, "sweeps must be >= 1");
    if (!(damping >= 0.0 && damping < 1.0)) return hgraph_fail(entry, "damping must lie in [0, 1)");
    if ((long long)N > 0x7fffffffffffffffLL / 8 / SA) return hgraph_fail(entry, "N * SA out of range");
    if ((long long)E > 0x7fffffffffffffffLL / 32 / SA) return hgraph_fail(entry, "2 * 2 E * SA out of range");
    if (E > 0 && (long long)sweeps > 0x7fffffffffffffffLL / 16 / E) return hgraph_fail(entry, "sweeps * 2 E out of range");
    if (N > 0 && (n_levels < 1 || n_levels > N)) return hgraph_fail(entry, "n_levels must lie in 1 .. N");
    if (N > 0 && (!score || !in_ptr || !level_ptr || !level_node || !level))
        return hgraph_fail(entry, "NULL pointer (score, in_ptr, level_ptr, level_node, level)");
    if (N > 0 && (!max_marginal || !decoded_state || !residual)) return hgraph_fail(entry, "NULL pointer (max_marginal, decoded_state, residual)");
    if (E > 0 && (!eu || !ev || !g || !d || !in_edge || !nu || !resid))
        return hgraph_fail(entry, "NULL pointer (eu, ev, g, d, in_edge, nu, resid)");
    if (N == 0) return GBP_OK;
    if (!graph_groups_fit(level_ptr, n_levels, N)) return hgraph_fail(entry, "level_ptr must start at 0, not decrease and end at N");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(horizon_graph::THREADS);
    const size_t half = (size_t)2 * E * SA;
    if (E > 0) {
        GBP_HIP(hipMemsetAsync(nu, 0, 2 * half * sizeof(double), st));
        const gbp_status rc = hgraph_sweeps<false>(N, E, S, has_absent, dz, switch_cost, eu, ev, score, g, d, in_ptr, in_edge, sweeps, damping, nu, resid, st);
        if (rc != GBP_OK) return rc;
    }
    hipLaunchKernelGGL(section::k_graph_residual, dim3((unsigned)sweeps), block, 0, st, 2LL * E, (const double*)resid, residual);
    GBP_HIP(hipGetLastError());
    const double* last = nu ? nu + (size_t)(sweeps & 1) * half : nu;
    hipLaunchKernelGGL(horizon_graph::k_hgraph_node<false>, dim3((unsigned)N), block, 0, st, E, SA, score, (const int*)in_ptr, (const int*)in_edge, last,
                       max_marginal, (int*)nullptr);
    GBP_HIP(hipGetLastError());
    for (int l = 0; l < n_levels; ++l) {
        const int count = level_ptr[l + 1] - level_ptr[l];
        if (count == 0) continue;
        hipLaunchKernelGGL(horizon_graph::k_hgraph_condition<false>, dim3((unsigned)count), block, 0, st, N, E, S, has_absent, dz, switch_cost,
                           (const int*)eu, (const int*)ev, score, g, d, (const int*)in_ptr, (const int*)in_edge, last, (const int*)level,
                           (const int*)level_node + level_ptr[l], count, (int*)decoded_state, (int*)nullptr, 0);
        GBP_HIP(hipGetLastError());
    }
    return GBP_OK;
}

// Coordinate ascent on the exact score of C horizons: per sweep one launch per colour of soundings, a workgroup for every (candidate,
// sounding of the colour).  All `refine` sweeps are launched; no counter is read on the host.  Every refusal comes before any launch.
extern "C" gbp_status gbp_horizon_graph_refine(int N, int E, int S, int has_absent, double dz, double switch_cost, int C, const int32_t* eu,
                                               const int32_t* ev, const double* score, const double* g, const double* d,
                                               const int32_t* in_ptr, const int32_t* in_edge, int n_colours, const int32_t* colour_ptr,
                                               const int32_t* colour_node, int refine, int32_t* state, int32_t* moves, void* stream)
{
    static const char* const entry = "gbp_horizon_graph_refine";
    if (const char* why = hgraph_refusal(N, E, S, has_absent, dz, switch_cost)) return hgraph_fail(entry, why);
    const int SA = S + has_absent;
    if (C < 1 || C > section::MAX_DRAWS + 1) return hgraph_fail(entry, "C must lie in 1 .. 65537");
    if (refine < 0 || refine > 65536) return hgraph_fail(entry, "refine must lie in 0 .. 65536");
    if ((long long)N > 0x7fffffffffffffffLL / 8 / SA) return hgraph_fail(entry, "N * SA out of range");
    if ((long long)C * N > 0x7fffffffLL) return hgraph_fail(entry, "C * N out of range");
    if (N > 0 && (n_colours < 1 || n_colours > N)) return hgraph_fail(entry, "n_colours must lie in 1 .. N");
    if (N > 0 && (!score || !in_ptr || !colour_ptr || !colour_node || !state))
        return hgraph_fail(entry, "NULL pointer (score, in_ptr, colour_ptr, colour_node, state)");
    if (N > 0 && refine > 0 && !moves) return hgraph_fail(entry, "moves is NULL");
    if (E > 0 && (!eu || !ev || !g || !d || !in_edge)) return hgraph_fail(entry, "NULL pointer (eu, ev, g, d, in_edge)");
    if (N == 0 || refine == 0) return GBP_OK;
    if (!graph_groups_fit(colour_ptr, n_colours, N)) return hgraph_fail(entry, "colour_ptr must start at 0, not decrease and end at N");
    hipStream_t st = (hipStream_t)stream;
    GBP_HIP(hipMemsetAsync(moves, 0, (size_t)C * refine * sizeof(int32_t), st));
    for (int t = 0; t < refine; ++t) {
        for (int c = 0; c < n_colours; ++c) {
            const int count = colour_ptr[c + 1] - colour_ptr[c];
            if (count == 0) continue;
            hipLaunchKernelGGL(horizon_graph::k_hgraph_condition<true>, dim3((unsigned)((long long)C * count)), dim3(horizon_graph::THREADS), 0, st, N, E,
                               S, has_absent, dz, switch_cost, (const int*)eu, (const int*)ev, score, g, d, (const int*)in_ptr, (const int*)in_edge,
                               (const double*)nullptr, (const int*)nullptr, (const int*)colour_node + colour_ptr[c], count, (int*)state,
                               (int*)moves + t, refine);
            GBP_HIP(hipGetLastError());
        }
    }
    return GBP_OK;
}

#include "gbp_horizon_draw.h"

// Joint draws of horizons (gbp_horizon_draw.h).  Along lines: the filter launch, one workgroup per sequence, then the walks, one
// workgroup per (sequence, 256 realisations).  On the survey graph: the same pair at the start sweep, then per sweep and colour a
// conditioned filter launch with a workgroup per (sequence, realisation) and a walk whose lanes read their own alpha rows.  Every
// refusal comes before any launch; no device array is read on the host.
namespace {

struct HorizonDrawArgs {
    int L;
    const int64_t* ptr;
    int64_t n_total;
    int E, S, has_absent;
    double dz;
    const double *score, *absent_score, *g, *d;
    double sw;
    const int32_t *step_edge, *eu, *ev, *cross_ptr, *cross_edge, *colour_ptr;
    const int64_t* row_key;
    uint64_t seed;
    int n_draws, first_draw;
    double *filtered, *scale;
    int32_t* draw_state;
};

// One filter launch and one walk launch: COND false draws every sequence alone from one shared alpha (lines NULL), COND true the
// sequences of `colour` given the other colours' states.
template <int NJ, bool COND>
gbp_status horizon_draw_pair(const HorizonDrawArgs& a, const int32_t* lines, int colour, unsigned sweep, hipStream_t st)
{
    const size_t lds = horizon_draw::filter_lds_doubles(a.S) * sizeof(double);
    const size_t walk_lds = horizon_draw::walk_lds_doubles(a.S, !COND) * sizeof(double);
    if (lds > 48 * 1024) {                                                  // (above the default limit of a launch's dynamic LDS)
        (void)hipFuncSetAttribute((const void*)horizon_draw::k_horizon_filter<NJ, COND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    if (walk_lds > 48 * 1024) {
        (void)hipFuncSetAttribute((const void*)horizon_draw::k_horizon_walk<!COND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)walk_lds);
        (void)hipGetLastError();
    }
    const unsigned filter_blocks = COND ? (unsigned)((long long)a.L * a.n_draws) : (unsigned)a.L;
    hipLaunchKernelGGL((horizon_draw::k_horizon_filter<NJ, COND>), dim3(filter_blocks), dim3(horizon_draw::THREADS), lds, st, (const long long*)a.ptr,
                       a.L, (long long)a.n_total, a.E, a.S, a.has_absent, a.dz, a.score, a.absent_score, a.g, a.d, a.sw, (const int*)a.step_edge,
                       (const int*)a.eu, (const int*)a.ev, (const int*)a.cross_ptr, (const int*)a.cross_edge, (const int*)a.colour_ptr,
                       (const int*)lines, colour, (const int*)a.draw_state, a.filtered, a.scale);
    GBP_HIP(hipGetLastError());
    hipLaunchKernelGGL((horizon_draw::k_horizon_walk<!COND>),
                       dim3((unsigned)a.L, (unsigned)((a.n_draws + horizon_draw::THREADS - 1) / horizon_draw::THREADS)), dim3(horizon_draw::THREADS),
                       walk_lds, st, (const long long*)a.ptr, a.L, (long long)a.n_total, a.E, a.S, a.has_absent, a.dz, a.g, a.d, a.sw,
                       (const int*)a.step_edge, (const int*)a.colour_ptr, (const int*)lines, colour, (const long long*)a.row_key,
                       (unsigned long long)a.seed, a.n_draws, a.first_draw, sweep, (const double*)a.filtered, (int*)a.draw_state);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

template <int NJ>
gbp_status horizon_draw_sweeps(const HorizonDrawArgs& a, const int32_t* colour_line, int n_colours, int first_sweep, int last_sweep, hipStream_t st)
{
    for (int t = first_sweep; t <= last_sweep; ++t) {
        if (t == 0) {                                                       // the start: every sequence alone
            const gbp_status rc = horizon_draw_pair<NJ, false>(a, nullptr, 0, 0u, st);
            if (rc != GBP_OK) return rc;
            continue;
        }
        for (int c = 0; c < n_colours; ++c) {
            const gbp_status rc = horizon_draw_pair<NJ, true>(a, colour_line, c, (unsigned)t, st);
            if (rc != GBP_OK) return rc;
        }
    }
    return GBP_OK;
}

gbp_status horizon_draw_dispatch(const HorizonDrawArgs& a, const int32_t* colour_line, int n_colours, int first_sweep, int last_sweep, hipStream_t st)
{
#define GBP_HORIZON_DRAW_CASE(nj) \
    case nj: return horizon_draw_sweeps<nj>(a, colour_line, n_colours, first_sweep, last_sweep, st)
    switch ((a.S + 1 + horizon::THREADS - 1) / horizon::THREADS) {
        GBP_HORIZON_DRAW_CASE(1);
        GBP_HORIZON_DRAW_CASE(2);
        GBP_HORIZON_DRAW_CASE(3);
        GBP_HORIZON_DRAW_CASE(4);
        GBP_HORIZON_DRAW_CASE(5);
        GBP_HORIZON_DRAW_CASE(6);
        GBP_HORIZON_DRAW_CASE(7);
        GBP_HORIZON_DRAW_CASE(8);
        default: return horizon_draw_sweeps<horizon::MAX_OWNED>(a, colour_line, n_colours, first_sweep, last_sweep, st);
    }
#undef GBP_HORIZON_DRAW_CASE
}

}  // namespace

extern "C" gbp_status gbp_horizon_draw(int L, const int64_t* ptr, int64_t total_n, int max_n, int S, double dz, const double* score,
                                       const double* absent_score, const double* g, const double* d, double switch_cost,
                                       const int64_t* row_key, uint64_t seed, int n_draws, double* filtered, double* scale,
                                       int32_t* draw_state, void* stream)
{
    if (L < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: L must be >= 0%s");
    if (S < 1 || S > horizon::MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: S must lie in 1 .. 2048 (the states live in LDS)%s");
    if (n_draws < 1 || n_draws > horizon_draw::MAX_DRAWS) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: n_draws must lie in 1 .. 65536%s");
    if (!(dz > 0.0) || !std::isfinite(dz)) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: dz must be positive and finite%s");
    if (!(switch_cost >= 0.0) || !std::isfinite(switch_cost)) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: switch must be >= 0 and finite%s");
    if (L == 0) return GBP_OK;
    if (total_n < 0 || max_n < 0 || max_n > total_n || total_n > (int64_t)max_n * L)
        return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: total_n and max_n do not fit L sequences%s");
    if (total_n == 0) return GBP_OK;                                        // (every sequence is empty)
    if (total_n > 0x7fffffffffffffffLL / 8 / (S + 1)) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: total_n * (S + 1) out of range%s");
    if (total_n > 0x7fffffffffffffffLL / 4 / n_draws) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: n_draws * total_n out of range%s");
    if (!ptr) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: ptr is NULL%s");
    if (!score || !g || !d) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: NULL pointer (score, g, d)%s");
    if (!filtered || !scale) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: NULL pointer (filtered, scale)%s");
    if (!draw_state) return fail(GBP_ERR_INVALID_ARG, "gbp_horizon_draw: draw_state is NULL%s");
    const HorizonDrawArgs a{L, ptr, total_n, 0, S, absent_score ? 1 : 0, dz, score, absent_score, g, d, switch_cost, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, row_key, seed, n_draws, 0, filtered, scale, draw_state};
    return horizon_draw_dispatch(a, nullptr, 0, 0, 0, (hipStream_t)stream);
}

extern "C" gbp_status gbp_horizon_graph_draw(int N, int E, int S, int has_absent, double dz, double switch_cost, const int32_t* eu,
                                             const int32_t* ev, const double* score, const double* g, const double* d, int L,
                                             const int64_t* ptr, const int32_t* step_edge, const int32_t* cross_ptr,
                                             const int32_t* cross_edge, int n_colours, const int32_t* colour_ptr,
                                             const int32_t* colour_line, const int64_t* row_key, uint64_t seed, int n_draws,
                                             int first_draw, int first_sweep, int sweeps, double* alpha, double* scale,
                                             int32_t* draw_state, void* stream)
{
    static const char* const entry = "gbp_horizon_graph_draw";
    if (const char* why = hgraph_refusal(N, E, S, has_absent, dz, switch_cost)) return hgraph_fail(entry, why);
    const int SA = S + has_absent;
    if (L < 0) return hgraph_fail(entry, "L must be >= 0");
    if (n_draws < 1 || n_draws > horizon_draw::MAX_DRAWS) return hgraph_fail(entry, "n_draws must lie in 1 .. 65536");
    if (first_draw < 0 || first_draw > horizon_draw::MAX_DRAWS - n_draws) return hgraph_fail(entry, "first_draw + n_draws must lie in 1 .. 65536");
    if (first_sweep < 0 || sweeps < first_sweep || sweeps > horizon_draw::MAX_SWEEPS)
        return hgraph_fail(entry, "the sweeps need 0 <= first_sweep <= sweeps <= 65535");
    if (N > 0 && L < 1) return hgraph_fail(entry, "soundings need a sequence (L >= 1)");
    if (L > 0 && (n_colours < 1 || n_colours > L)) return hgraph_fail(entry, "the colour lists must cover the sequences: n_colours must lie in 1 .. L");
    if ((long long)n_draws * N > 0x7fffffffffffffffLL / 8 / SA) return hgraph_fail(entry, "n_draws * N * SA out of range");
    if ((long long)n_draws * N > 0x7fffffffffffffffLL / 4) return hgraph_fail(entry, "n_draws * N out of range");
    if ((long long)L * n_draws > 0x7fffffffLL) return hgraph_fail(entry, "L * n_draws out of range");
    if (N > 0 && (!score || !ptr || !step_edge || !cross_ptr || !colour_ptr || !colour_line))
        return hgraph_fail(entry, "NULL pointer (score, ptr, step_edge, cross_ptr, colour_ptr, colour_line)");
    if (N > 0 && (!alpha || !scale || !draw_state)) return hgraph_fail(entry, "NULL pointer (alpha, scale, draw_state)");
    if (E > 0 && (!eu || !ev || !g || !d || !cross_edge)) return hgraph_fail(entry, "NULL pointer (eu, ev, g, d, cross_edge)");
    if (N == 0) return GBP_OK;
    const HorizonDrawArgs a{L, ptr, N, E, S, has_absent, dz, score, nullptr, g, d, switch_cost, step_edge, eu, ev, cross_ptr, cross_edge, colour_ptr,
                            row_key, seed, n_draws, first_draw, alpha, scale, draw_state};
    return horizon_draw_dispatch(a, colour_line, n_colours, first_sweep, sweeps, (hipStream_t)stream);
}

#include "gbp_section_graph_draw.h"

// Joint draws across lines (gbp_section_graph_draw.h): K unless the caller has it, the weights, then per sweep a filter launch and a draw
// launch -- over every sequence at the start sweep, per colour class afterwards.  A launch holds a block for every (sequence, realisation)
// and the blocks past the colour's own sequences leave at once: colour_ptr stays on the device.  Every refusal comes before any launch;
// no device array is read on the host.
extern "C" gbp_status gbp_section_graph_draw(int S, int E, int n, int L, const int64_t* ptr, const int32_t* eu, const int32_t* ev,
                                             const int32_t* n_used, const double* score, const double* g, const double* d2,
                                             int kernel_ready, double* K, const int32_t* step_edge, const int32_t* cross_ptr,
                                             const int32_t* cross_edge, int n_colours, const int32_t* colour_ptr,
                                             const int32_t* colour_line, const int64_t* row_key, uint64_t seed, int n_draws,
                                             int first_draw, int first_sweep, int last_sweep, double* w, double* filtered, double* scale,
                                             int32_t* draw_state, void* stream)
{
    if (S < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: S must be >= 0%s");
    if (E < 0 || E > 0x3fffffff) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: E must lie in 0 .. 2^30 - 1%s");
    if (n < 1 || n > section::GRAPH_MAX_STATES) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: n must lie in 1 .. 256%s");
    if (L < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: L must be >= 0%s");
    if (n_draws < 1 || n_draws > section::MAX_DRAWS) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: n_draws must lie in 1 .. 65536%s");
    if (first_draw < 0 || first_draw > section::MAX_DRAWS - n_draws)
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: first_draw + n_draws must lie in 1 .. 65536%s");
    if (first_sweep < 0 || last_sweep < first_sweep || last_sweep > 65535)
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: the sweeps need 0 <= first_sweep <= last_sweep <= 65535%s");
    if (E > 0 && S < 2) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: an edge needs two soundings%s");
    if (S > 0 && L < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: soundings need a sequence (L >= 1)%s");
    if (L > 0 && (n_colours < 1 || n_colours > L)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: n_colours must lie in 1 .. L%s");
    // (E n n and n_draws S n doubles fit 63 bits under the limits above; the grid of the filter is what can overflow)
    if ((long long)L * n_draws > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: L * n_draws out of range%s");
    if (S > 0 && (!ptr || !n_used || !score || !step_edge || !cross_ptr || !colour_ptr || !colour_line))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: NULL pointer (ptr, n_used, score, step_edge, cross_ptr, colour_ptr, colour_line)%s");
    if (S > 0 && (!w || !filtered || !scale || !draw_state))
        return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: NULL pointer (w, filtered, scale, draw_state)%s");
    if (E > 0 && (!eu || !ev || !K || !cross_edge)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: NULL pointer (eu, ev, K, cross_edge)%s");
    if (E > 0 && !kernel_ready && (!g || !d2)) return fail(GBP_ERR_INVALID_ARG, "gbp_section_graph_draw: NULL pointer (g, d2) without kernel_ready%s");
    if (S == 0) return GBP_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(section::THREADS);
    if (E > 0 && !kernel_ready) {
        hipLaunchKernelGGL(section::k_graph_kernel, dim3((unsigned)E), block, 0, st, S, n, (const int*)eu, (const int*)ev, (const int*)n_used, g, d2, K);
        GBP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(section::k_graph_weights, dim3((unsigned)S), block, 0, st, n, (const int*)n_used, score, w);
    GBP_HIP(hipGetLastError());
    const size_t lds = section::lds_bytes(n);
    const dim3 grid_filter((unsigned)((long long)L * n_draws)), grid_draw((unsigned)((long long)L * ((n_draws + 63) / 64)));
#define GBP_GRAPH_DRAW(COND, LINES, COLOUR, SWEEP)                                                                                        \
    hipLaunchKernelGGL((section::k_graph_line_filter<COND>), grid_filter, block, lds, st, S, E, n, L, (const long long*)ptr, (const int*)eu,  \
                       (const int*)ev, (const int*)n_used, (const double*)w, (const double*)K, (const int*)step_edge, (const int*)cross_ptr,  \
                       (const int*)cross_edge, (const int*)colour_ptr, (const int*)(LINES), COLOUR, (const int*)draw_state, filtered, scale); \
    GBP_HIP(hipGetLastError());                                                                                                           \
    hipLaunchKernelGGL(section::k_graph_line_draw, grid_draw, dim3(64), 0, st, S, E, n, L, (const long long*)ptr, (const int*)n_used,         \
                       (const double*)K, (const int*)step_edge, (const int*)colour_ptr, (const int*)(LINES), COLOUR,                          \
                       (const long long*)row_key, (unsigned long long)seed, n_draws, first_draw, (unsigned)(SWEEP),                           \
                       (const double*)filtered, (int*)draw_state);                                                                        \
    GBP_HIP(hipGetLastError())
    for (int t = first_sweep; t <= last_sweep; ++t) {
        if (t == 0) {                                                       // the start: every sequence alone
            GBP_GRAPH_DRAW(false, nullptr, 0, 0);
            continue;
        }
        for (int c = 0; c < n_colours; ++c) {
            GBP_GRAPH_DRAW(true, colour_line, c, t);
        }
    }
#undef GBP_GRAPH_DRAW
    return GBP_OK;
}

#include "gbp_bodies.h"

// Connected bodies (gbp_bodies.h): one launch, one workgroup per (realisation, group).  group_ptr, eu and ev are device arrays that the
// kernel reads; the entry copies them to the host first, behind the stream's earlier work, because an edge that does not fit would be
// followed outside the outputs: every refusal comes before the launch.
extern "C" gbp_status gbp_bodies_label(int R, int S, int C, int E, int G, const int64_t* group_ptr, const int32_t* eu, const int32_t* ev,
                                       const double* raster, double lo, double hi, const double* a, const double* t, double unit,
                                       int32_t* label, int32_t* cells, int64_t* measure_q, int32_t* sweeps, void* stream)
{
    if (R < 1 || R > bodies::MAX_REALISATIONS) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: R must lie in 1 .. 65536%s");
    if (S < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: S must be >= 0%s");
    if (C < 1 || C > bodies::MAX_COLUMNS) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: C must lie in 1 .. 4096%s");
    if (E < 0 || E > 0x3fffffff) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: E must lie in 0 .. 2^30 - 1%s");
    if (G < 0 || G > S) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: G must lie in 0 .. S%s");
    if ((long long)R * S * C > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: R * S * C must be below 2^31%s");
    if (E > 0 && S < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: an edge needs a sounding%s");
    if (S > 0 && G < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: soundings need a group (G >= 1)%s");
    if ((a == nullptr) != (t == nullptr)) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: a and t are given together or not at all%s");
    if (a && !(unit > 0.0 && unit <= 1.7976931348623157e308)) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: unit must be finite and > 0%s");
    if (S > 0 && (!group_ptr || !raster || !label || !cells || !sweeps))
        return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: NULL pointer (group_ptr, raster, label, cells, sweeps)%s");
    if (S > 0 && a && !measure_q) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: NULL pointer (measure_q with a and t)%s");
    if (E > 0 && (!eu || !ev)) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: NULL pointer (eu, ev)%s");
    if (S == 0) return GBP_OK;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> gp((size_t)G + 1);
    std::vector<int32_t> hu((size_t)E), hv((size_t)E);
    GBP_HIP(hipMemcpyAsync(gp.data(), group_ptr, gp.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (E > 0) {
        GBP_HIP(hipMemcpyAsync(hu.data(), eu, hu.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        GBP_HIP(hipMemcpyAsync(hv.data(), ev, hv.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    GBP_HIP(hipStreamSynchronize(st));
    if (gp[0] != 0 || gp[(size_t)G] != S) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: group_ptr must start at 0 and end at S%s");
    for (int g = 0; g < G; ++g)
        if (gp[(size_t)g + 1] < gp[(size_t)g]) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: group_ptr must not decrease%s");
    int g = 0;                                                              // the group of the edge before: the edges come group by group
    for (int e = 0; e < E; ++e) {
        const long long u = hu[(size_t)e], v = hv[(size_t)e];
        if (u < 0 || u >= S || v < 0 || v >= S) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: an edge's sounding lies outside 0 .. S - 1%s");
        if (u < gp[(size_t)g]) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: the edges must be sorted by the group of eu%s");
        while (u >= gp[(size_t)g + 1]) ++g;                                 // (u < S = gp[G]: it ends)
        if (v < gp[(size_t)g] || v >= gp[(size_t)g + 1]) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: an edge joins two groups%s");
    }
    if ((long long)R * G > 0x7fffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_bodies_label: R * G out of range%s");
    const dim3 grid((unsigned)((long long)R * G)), block(bodies::THREADS);
    if (a)
        hipLaunchKernelGGL(bodies::k_bodies_label<true>, grid, block, 0, st, S, C, E, G, (const long long*)group_ptr, (const int*)eu, (const int*)ev,
                           raster, lo, hi, a, t, unit, (int*)label, (int*)cells, (long long*)measure_q, (int*)sweeps);
    else
        hipLaunchKernelGGL(bodies::k_bodies_label<false>, grid, block, 0, st, S, C, E, G, (const long long*)group_ptr, (const int*)eu, (const int*)ev,
                           raster, lo, hi, a, t, unit, (int*)label, (int*)cells, (long long*)nullptr, (int*)sweeps);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}

#include "gbp_boreholes.h"

// Borehole logs as a score of the kept models (gbp_boreholes.h): one launch, one wave per (sounding, 64 models).  att_ptr, att_bore,
// bore_ptr and cls are device arrays that the kernel follows; the entry copies them to the host first, behind the stream's earlier
// work, as gbp_bodies_label does with its edges: every refusal comes before the launch.
extern "C" gbp_status gbp_borehole_score(int S, int n_slots, int K, const int32_t* ens_k, const double* ens_edges, const double* ens_sigma,
                                         int n, const int32_t* rows, const int32_t* n_used, int A, const int32_t* att_ptr,
                                         const int32_t* att_bore, const double* att_var, const double* att_shift, int Nb,
                                         const int32_t* bore_ptr, int I, const double* top, const double* bottom, const double* value,
                                         const double* sd, const int32_t* cls, int C, const double* class_mean, const double* class_scale,
                                         const double* class_ln_prior, double class_floor, double* score, double* part, int32_t* skipped,
                                         void* stream)
{
    using namespace boreholes;
    if (S < 0 || n_slots < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: negative or zero size%s");
    if (n < 1 || n > MAX_MODELS) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: n outside 1 .. 1024%s");
    if (K < 1 || K > MAX_K) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: K outside 1 .. 64%s");
    if (C < 0 || C > MAX_CLASSES) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: C outside 0 .. 16%s");
    if (A < 0 || Nb < 0 || I < 0) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: A, Nb and I must be >= 0%s");
    if (A > 0 && Nb < 1) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: an attachment needs a borehole%s");
    if (!(class_floor > 0.0 && class_floor < 1.0)) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: class_floor must lie in (0, 1)%s");
    if (C > 0 && (!class_mean || !class_scale || !class_ln_prior))
        return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: NULL pointer (class_mean, class_scale, class_ln_prior)%s");
    for (int c = 0; c < C; ++c) {
        if (!std::isfinite(class_mean[c]) || !std::isfinite(class_ln_prior[c]))
            return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: every class mean and log prior must be finite%s");
        if (!(std::isfinite(class_scale[c]) && class_scale[c] > 0.0))
            return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: every class scale must be finite and positive%s");
    }
    const int chunks = (n + WAVE - 1) / WAVE;
    if ((int64_t)S * chunks * WAVE > 0xffffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: S * waves out of range (more than 2^32 - 1 threads)%s");
    if ((int64_t)A * n > 0x7fffffffffffLL) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: A * n out of range%s");
    if (S == 0) return GBP_OK;                     // (an empty block: empty device arrays have no address)
    if (!ens_k || !ens_edges || !ens_sigma || !rows || !n_used || !att_ptr || !score)
        return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: NULL pointer (ens_k, ens_edges, ens_sigma, rows, n_used, att_ptr, score)%s");
    if (A > 0 && (!att_bore || !att_var || !att_shift || !bore_ptr))
        return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: NULL pointer (att_bore, att_var, att_shift, bore_ptr)%s");
    if (A > 0 && I > 0 && (!top || !bottom || !value || !sd || !cls))
        return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: NULL pointer (top, bottom, value, sd, cls)%s");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> ap((size_t)S + 1), ab((size_t)A), bp(A > 0 ? (size_t)Nb + 1 : 0), hc(A > 0 ? (size_t)I : 0);
    GBP_HIP(hipMemcpyAsync(ap.data(), att_ptr, ap.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (A > 0) {
        GBP_HIP(hipMemcpyAsync(ab.data(), att_bore, ab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        GBP_HIP(hipMemcpyAsync(bp.data(), bore_ptr, bp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (I > 0) GBP_HIP(hipMemcpyAsync(hc.data(), cls, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    GBP_HIP(hipStreamSynchronize(st));
    if (ap[0] != 0 || ap[(size_t)S] != A) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: att_ptr must start at 0 and end at A%s");
    for (int s = 0; s < S; ++s)
        if (ap[(size_t)s + 1] < ap[(size_t)s]) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: att_ptr must not decrease%s");
    if (A > 0) {
        if (bp[0] != 0 || bp[(size_t)Nb] != I) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: bore_ptr must start at 0 and end at I%s");
        for (int b = 0; b < Nb; ++b)
            if (bp[(size_t)b + 1] < bp[(size_t)b]) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: bore_ptr must not decrease%s");
        for (int e = 0; e < A; ++e)
            if (ab[(size_t)e] < 0 || ab[(size_t)e] >= Nb) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: an attachment's borehole lies outside 0 .. Nb - 1%s");
        for (int i = 0; i < I; ++i)
            if (hc[(size_t)i] < -1 || hc[(size_t)i] >= C) return fail(GBP_ERR_INVALID_ARG, "gbp_borehole_score: an interval's class lies outside -1 .. C - 1%s");
    }
    ScoreArgs a = {};
    a.S = S; a.n_slots = n_slots; a.K = K; a.n = n; a.C = C; a.chunks = chunks;
    a.ens_k = ens_k; a.ens_edges = ens_edges; a.ens_sigma = ens_sigma; a.rows = rows; a.n_used = n_used;
    a.att_ptr = att_ptr; a.att_bore = att_bore; a.att_var = att_var; a.att_shift = att_shift; a.bore_ptr = bore_ptr;
    a.top = top; a.bottom = bottom; a.value = value; a.sd = sd; a.cls = cls;
    for (int c = 0; c < C; ++c) { a.mean[c] = class_mean[c]; a.scale[c] = class_scale[c]; a.ln_prior[c] = class_ln_prior[c]; }
    a.floor = class_floor; a.score = score; a.part = part; a.skipped = skipped;
    hipLaunchKernelGGL(k_borehole_score, dim3((unsigned)((int64_t)S * chunks)), dim3(WAVE), lds_bytes(K), st, a);
    GBP_HIP(hipGetLastError());
    return GBP_OK;
}
