// kernels.hip.h — gfx950 (CDNA4, wave64) device code of libroman_hip.so.
//
// Pipeline for a batch of B independent submap pairs (one "problem" each):
//   k_cos_*      normalised cosine matrix (+ descriptor norms), f64 MFMA 16x16x4   (cos_feature_dim > 0)
//   k_tables     intra-map distance tables with NaN sentinels      (n1^2 + n2^2 entries)
//   k_live       single scores + ordered compaction of live associations; picks the problem's KIND
//   k_rowbase / k_items   prefix of live counts over problems, work-item list
//   k_count      the O(L^2) pair tests -> candidate bit matrix (upper 64-bit words), k_mirror the lower ones
//   k_rowprefix  row degrees (+ per-word prefix counts for the fallback layout)
//   k_rowsort    rows by descending degree (+ kind 0: offsets of the candidate lists)
//   kind 0 ("stream", L <= STREAM_MAXL):
//     k_upper      every candidate pair kept once, in the row of its endpoint with the smaller POSITION (rank by degree):
//                  the row's kept candidates as a list of 16-bit live column indices
//     k_slicegeom  slice widths / bases of the quad layout
//     k_fill_list  candidate lists -> values, one list quad (4 entries) per lane at a time, straight into the layout
//     k_solve_up   persistent per-problem CLIPPER solve on the upper triangle (pull + push SpMV)
//   kind 1 (fallback, any L): symmetric sorted SELL-64 in live numbering: k_fill, then k_solve (a workgroup per
//     problem) or k_solve_wide (cooperative launch: the whole device on one large problem at a time, or teams of compute
//     units — the workgroups of an XCD or of half an XCD — on one problem each)
//   kind 2: skipped for lack of workspace (k_skipped writes ROMAN_ST_WORKSPACE)
//   kind 3: finished by k_small — batch calls, <= 128 live associations (the reference's demo scale): pair tests, positions,
//     values, solve and pose in ONE kernel right behind k_live; the kernels above pass such a problem by
//   (k_cos_wave: the cosine matrices of maps of at most 48 objects, one wave per problem)
//
// Matrix layout of kind 0: only the strict upper triangle of M in position numbering is stored
// (entry (p,q), p < q, in row p) — 10 bytes per non-zero of the upper triangle.  Rows are cut into slices of 64
// consecutive positions, a slice is padded to its longest row (multiple of 4 entries) and stored as "quads":
// the 4 column indices of entries 4g..4g+3 of a lane are one 8-byte word, the values of entries 2h,2h+1 one
// 16-byte pair: 3 wide, fully coalesced loads per 4 entries.  Padding is inert (value 0, column L + lane, C-flag).
// Layout of kind 1 (sorted SELL-64, both triangles): entry e of the row in slot (slice s, lane l) sits at
//      sliceBase[s] + e*64 + l .
#pragma once
#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/roman_hip.h"

namespace roman {

constexpr int WAVE = 64;
constexpr int STREAM_MAXL = 3072;        // live associations the stream layout / solver serve (48 slices of 64 rows)

struct DevParams {
    roman_params_t p;
    double sig2;        // sigma^2
    double sin_unc;     // sin(gravity_unc_ang_rad)
    double x_eps;       // smallest x with sqrt(x) >= epsilon   (c < eps  <=>  c*c-sum < x_eps)
    double x_mindist;   // smallest x with sqrt(x) >= mindist   (l < mindist <=> l^2 < x_mindist)
    int32_t single;     // invariant has per-association scores
    int32_t gravity;    // ROMAN invariant && gravity_guided
    int32_t F;          // features per object
    int32_t max_compact; // streaming solver: column compactions allowed per problem (speed only; set per launch)
    int32_t gmode;      // 0: no gravity; 1 + ROMAN_GRAV_* otherwise (1 combined, 2 separate gates, 3 z gate on full lengths)
    int32_t diag_one;   // single scores present but the diagonal is the identity (ROMAN_SINGLE_OFFDIAG)
    int32_t keep_all;   // single scores present but a zero one removes nothing (ROMAN_SINGLE_DIAG_KEEP): every association is live
    int32_t pruned;     // ROMAN_INV_EUCLIDEAN_PRUNED: the single score is the 0/1 prefilter on the RAW descriptor product; pair score alone in M,
                        // identity diagonal; a problem in which nothing survives keeps every association; rounding over survivors only
    int32_t allow_fallback;  // the fallback kernels are part of this launch; otherwise a problem that does not fit the stream layout is
                             // SKIPPED (kind 2, ROMAN_ST_WORKSPACE) and runs again with them (set per launch, from the sizing history)
    int32_t wide;            // fallback problems of this launch go to k_solve_wide (few, large) instead of k_solve (set per launch)
    int32_t idx16;           // ... and their column labels are 16 bits wide (no C flag; 0xffff = inert): 10 instead of 12 bytes per entry
    int32_t small_only;      // the general kernels are NOT part of this launch (every problem of this parameter block has so far been finished by
                             // k_small): a problem k_small leaves behind is skipped (kind 2, ROMAN_ST_WORKSPACE) and takes them on its second run
    int32_t stream_maxL;     // problems of up to this many live associations take the stream layout (<= STREAM_MAXL; set per launch:
                             // it is also the column capacity of k_fill_slice's LDS tile and of the stream solver's LDS vectors)
    int32_t pre_K;           // k_count's integer prefilter: a pair goes to the exact gate iff its two quantised table entries differ by at most pre_K bins
    int32_t plain_all;       // plain-CLIPPER view of a scored matrix (roman_mno_batch*): an association with a zero single score stays a NODE — live, with
                             // an empty row (fuse_pair gives its pairs the value 0: inert slots) and, like every node of the view, a unit diagonal (diag_one)
    double  pre_invw;        // ... bins per metre (1 / bin width; bin width = epsilon / 32)
};

struct ProbDesc {
    int64_t off1, off2;    // first object of map 1 / map 2 in the feature pool
    int64_t assocOff;      // row offset into the explicit association list, -1 = all-to-all
    int64_t liveOff;       // offset into pools with one slot per input association
    int64_t cosOff;        // offset into the cosine pool (n1*n2)
    int64_t tabOff;        // offset into the table pool (n1*n1 then n2*n2)
    int64_t normOff;       // offset into the norm pool (n1 then n2)
    int32_t n1, n2, nA;
    int32_t qtabOff4;      // offset into the pool of 16-bit table bins (k_count's prefilter), in units of four entries: n1 rows of (n1 + 3 & ~3), then n2 rows of (n2 + 3 & ~3)
};

struct ProbState {
    int32_t  L;            // live associations
    int32_t  rowBase;      // prefix of L over the batch
    int64_t  nnzOff;       // offset of this problem's matrix segment
    int64_t  maskOff;      // offset (in 64-bit words) of this problem's candidate bit matrix
    uint32_t nnzCap;       // padded SELL slots allocated for this problem
    int32_t  itemBase;     // first work item (row block) of this problem
    int32_t  sgBase;       // first slice group (k_fill_slice work item) of this problem
    int32_t  kind;         // 0: stream layout + k_solve_up (L <= STREAM_MAXL), 1: symmetric SELL-64 fallback
    unsigned long long nnzUpper;   // stored strict-upper non-zeros (after the affinityeps filter)
    int64_t  listOff;      // stream layout: first element of this problem's candidate lists in the list pool
};

struct BatchTotals {
    int64_t nnzTotal;      // sum of nnzCap over the problems that fit
    int64_t maskWords;     // sum over the problems that fit of L * ceil(L/64)
    int32_t R;             // sum of L
    int32_t maxL;
    int32_t items;         // work items (row blocks) of the pair-test / fill kernels
    int32_t sliceGroups;   // work items (groups of SPI slices) of k_fill_slice
    // what the whole batch WOULD need (the pools are sized before the live counts are known: problems that do not fit
    // are skipped with ROMAN_ST_WORKSPACE and the host grows the pools from these numbers)
    int64_t needMaskWords;
    int64_t needNnz;
    int32_t overflow;      // problems skipped for lack of workspace
    int32_t maxStreamL;    // largest L among stream-layout problems
    int32_t minStreamL;    // smallest L among stream-layout problems (does the small-problem solver have work?)
    int32_t nGeneral;      // problems left to the general kernels (not finished by k_small, not skipped)
    unsigned long long listTop;    // bump pointer of the candidate-list pool = what the whole batch needs of it
    int32_t cosScreened;   // problems whose cosines went through k_cos_sel (0: the dense kernels took the batch) ...
    int32_t cosDense;      // ... and how many of them it left to the dense kernel (more candidates than its list holds)
};

struct ItemDesc { int32_t b, row0; };   // a block of consecutive live rows of problem b

// column-index word of a stored entry: live column index + a flag bit "C_pq == 0"
template <typename IdxT> struct IdxTraits;
template <> struct IdxTraits<uint16_t> { static constexpr uint32_t CZ = 0x8000u; static constexpr uint32_t MASK = 0x7fffu; };
template <> struct IdxTraits<uint32_t> { static constexpr uint32_t CZ = 0x80000000u; static constexpr uint32_t MASK = 0x7fffffffu; };

// Fallback layout, column word of an inert entry (padding / filtered): 32-bit words carry the row's own position with the C
// flag (a real vector element, excluded from C); 16-bit words (k_solve_wide only, no flag bit) are 0xffff = "no column".
template <typename IdxT> __device__ __forceinline__ IdxT fb_inert(uint32_t pos)
{
    return sizeof(IdxT) == 2 ? (IdxT)0xffffu : (IdxT)(pos | IdxTraits<IdxT>::CZ);
}

// Position of entry e of the row in lane-slot `slot` of a slice that starts at element `sbase` of the
// problem's matrix segment (sbase is a multiple of 256 in the quad layout, of 64 otherwise).
//  - SELL-64 (QUAD == false):  sbase + e*64 + slot  for both arrays.
//  - quad layout (QUAD == true, 16-bit indices, widths multiples of 4): the 4 column indices of entries
//    4g..4g+3 of a lane are contiguous (one 8-byte load), the values of entries 2h, 2h+1 are contiguous
//    (one 16-byte load): 3 wide loads per 4 entries instead of 8 narrow ones.
template <bool QUAD> __device__ __forceinline__ int64_t col_pos(int64_t sbase, uint32_t slot, uint32_t e)
{
    return QUAD ? sbase + (int64_t)(e >> 2) * 256 + slot * 4 + (e & 3u) : sbase + (int64_t)e * 64 + slot;
}
template <bool QUAD> __device__ __forceinline__ int64_t val_pos(int64_t sbase, uint32_t slot, uint32_t e)
{
    return QUAD ? sbase + (int64_t)(e >> 1) * 128 + slot * 2 + (e & 1u) : sbase + (int64_t)e * 64 + slot;
}

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------

__device__ __forceinline__ double d_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }    // wave-uniform value into an SGPR

// association index p of problem pd -> (map-1 object, map-2 object)
__device__ __forceinline__ void decode_assoc(const ProbDesc& pd, const int32_t* __restrict__ assoc,
                                             int p, int& i, int& j)
{
    if (pd.assocOff >= 0) { i = assoc[2 * (pd.assocOff + p)]; j = assoc[2 * (pd.assocOff + p) + 1]; }
    else { i = p / pd.n2; j = p - i * pd.n2; }
}

// exp and cbrt as FIXED sequences of correctly-rounded operations: the `score > affinityeps`
// gate is applied after them, so they must produce the same bits as the oracle's oracle_exp()/oracle_cbrt()
// (oracle/clipper_oracle.c states the same sequences; tests/test_gpu_parity.py compares the bits).  < 1 ulp.
__device__ __forceinline__ double bits_f64(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ double fx_exp(double y)
{
    if (!(y > -700.0 && y < 700.0)) return exp(y);
    constexpr double LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
    const double k = rint(y * LOG2E);
    const double r1 = fma(-k, LN2_HI, y);
    const double rl = -k * LN2_LO;
    const double r = r1 + rl;
    const double r_err = (r1 - r) + rl;
    double q = 0x1.6124613a86d09p-33;                              // 1/13!
    q = fma(q, r, 0x1.1eed8eff8d898p-29); q = fma(q, r, 0x1.ae64567f544e4p-26); q = fma(q, r, 0x1.27e4fb7789f5cp-22);
    q = fma(q, r, 0x1.71de3a556c734p-19); q = fma(q, r, 0x1.a01a01a01a01ap-16); q = fma(q, r, 0x1.a01a01a01a01ap-13);
    q = fma(q, r, 0x1.6c16c16c16c17p-10); q = fma(q, r, 0x1.1111111111111p-7);  q = fma(q, r, 0x1.5555555555555p-5);
    q = fma(q, r, 0x1.5555555555555p-3);  q = fma(q, r, 0.5);     // ... 1/2!
    const double a = 1.0 + r;
    const double a_err = (r - (a - 1.0)) + r_err;
    const double p = a + fma(r * r, q, a_err);
    return p * bits_f64((unsigned long long)(1023 + (int)k) << 52);
}
__device__ __forceinline__ double fx_cbrt(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const int E = (int)((b >> 52) & 0x7ffull);
    if (!(x > 0.0) || E == 0 || E == 0x7ff) return cbrt(x);
    constexpr double C0 = 0x1.331e76e38c2bfp+0, C1 = -0x1.142641324f5d9p-2, C2 = 0x1.49dcf893faf42p-5, C3 = -0x1.2190c96665e59p-9;
    constexpr double THIRD = 0x1.5555555555555p-2;
    const int e = E - 1023;
    const int q = (e >= 0) ? e / 3 : -((2 - e) / 3);
    const int rem = e - 3 * q;
    const double m = bits_f64((b & 0x000fffffffffffffull) | ((unsigned long long)(1023 + rem) << 52));
    double y = fma(fma(fma(C3, m, C2), m, C1), m, C0);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const double y2 = y * y, y3 = y2 * y;
        const double w = fma(-m, y3, 4.0);
        y = (y * w) * THIRD;
    }
    const double yy = y * y;
    double t = m * yy;
    const double t2 = t * t, e2 = fma(t, t, -t2);
    const double r = fma(-e2, t, fma(-t2, t, m));
    t = fma(r, yy * THIRD, t);
    return t * bits_f64((unsigned long long)(1023 + q) << 52);
}

__device__ __forceinline__ double root_w(double x, double w)
{
    if (w == 1.0) return x;
    if (w == 2.0) return sqrt(x);
    if (w == 3.0) return fx_cbrt(x);
    if (w == 4.0) return sqrt(sqrt(x));
    if (w == 6.0) return fx_cbrt(sqrt(x));
    return pow(x, 1.0 / w);
}
__device__ __forceinline__ double pow_w(double x, double w) { return (w == 1.0) ? x : pow(x, w); }

// Single score of one association; mirrors oracle single_score() operation for operation.
// ra(f), rb(f): ratio feature f of the two objects.
template <class RA, class RB>
__device__ __forceinline__ double single_score(const DevParams& D, RA ra, RB rb, double cosv)
{
    const roman_params_t& P = D.p;
    const int Fr = P.ratio_feature_dim, Fc = P.cos_feature_dim;
    if (D.pruned) {                         // the reference's NumPy prefilter ([REF roman/align/dist_reg_with_pruning.py:75-90]) as a 0/1 score;
        if (Fc > 0 && cosv < P.cosine_min) return 0.0;          // cosv is the RAW product here; a NaN compares false = keeps, as in NumPy
        for (int f = 0; f < Fr; ++f) {
            const double a = ra(f), b = rb(f);
            const double mn = a < b ? a : b, mx = a < b ? b : a;
            if (mn / mx < P.ratio_epsilon[f]) return 0.0;
        }
        return 1.0;
    }
    double wsum = 0.0, prod = 1.0, asum = 0.0;
    if (Fr > 0) {
        double rp = 1.0;
        for (int f = 0; f < Fr; ++f) {
            const double a = ra(f), b = rb(f);
            const double mn = a < b ? a : b, mx = a < b ? b : a;
            const double r = (mx > 0.0) ? mn / mx : 1.0;
            if (r < P.ratio_epsilon[f]) return 0.0;
            rp *= r;
        }
        const double R = root_w(rp, (double)Fr);
        prod *= pow_w(R, P.ratio_weight); asum += P.ratio_weight * R; wsum += P.ratio_weight;
    }
    if (Fc > 0) {
        double c = (cosv - P.cosine_min) / (P.cosine_max - P.cosine_min);
        if (!(c > 0.0)) return 0.0;
        if (c > 1.0) c = 1.0;
        prod *= pow_w(c, P.cosine_weight); asum += P.cosine_weight * c; wsum += P.cosine_weight;
    }
    if (wsum == 0.0) return 1.0;
    switch (P.fusion_method) {
    case ROMAN_FUSE_ARITHMETIC_MEAN: return asum / wsum;
    case ROMAN_FUSE_PRODUCT:         return prod;
    default:                         return root_w(prod, wsum);
    }
}

// Fusion of the pair score with the two single scores; mirrors oracle fuse_pair().
__device__ __forceinline__ double fuse_pair(const DevParams& D, double sa, double sp, double sq)
{
    if (!D.single || D.keep_all) return sa;
    if (sa == 0.0 || sp == 0.0 || sq == 0.0) return 0.0;
    if (D.pruned) return sa;
    if (D.p.single_mode == ROMAN_SINGLE_DIAG) return sa;
    const double ss = sp * sq, wd = D.p.distance_weight;
    switch (D.p.fusion_method) {
    case ROMAN_FUSE_ARITHMETIC_MEAN: return (wd * sa + (sp + sq)) / (wd + 2.0);
    case ROMAN_FUSE_PRODUCT:         return sa * ss;
    default:                         return root_w(pow_w(sa, wd) * ss, wd + 2.0);
    }
}

// ---------------------------------------------------------------------------------------------
// The cosine kernels: cos[i][j] = <d1_i, d2_j> / (|d1_i| |d2_j|) on the f64 matrix core (v_mfma_f64_16x16x4_f64).
// Operand layout of one MFMA: lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]; result reg r of lane l is
// C[row = (l>>4) + 4r][col = l&15].  Per 16 descriptor elements a lane holds 4 CONSECUTIVE doubles of each of its rows and
// feeds element t of them to MFMA t: MFMA t contracts k = k0 + 4*(l>>4) + t — any bijection k <-> (MFMA, l>>4) is a valid
// contraction order as long as A and B use the same one.  Every kernel below keeps this one order (chunks of 16 ascending,
// then t = 0..3) and the same order of the norm sums — "k_cos's own" in their comments, after the first kernel that had it
// (one 32x32 tile per wave, operands from global memory; retired: DESIGN.md) — so all of them give identical bits.
// ---------------------------------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double dbl2_t __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(8))) d4u_t { double v[4]; };     // 8-byte aligned 32-byte load

// ---------------------------------------------------------------------------------------------
// k_cos_wave: the reference's DEMO scale (submaps of at most 48 objects): ONE WAVE computes a problem's whole cosine matrix —
// up to 3 x 3 MFMA blocks in registers, operands straight from global memory with 32-byte loads (the descriptors of a few
// hundred small submaps are L2-resident), no LDS, no barrier.  k_cos_tile gives such a problem a 4-wave workgroup that
// meets at a barrier 48 times (768-d descriptors) to multiply at most 9 blocks: 0.32 ms per 4096 problems, three times the
// matrix pipe's own time.  Per 16 descriptor elements a lane loads 4 consecutive doubles of each of its <= 3 + 3 rows and
// feeds element t of every load to the MFMAs of step t: the contraction order of every output element — chunks of 16
// ascending, step t of a chunk contracts k = k0 + 4 * (lane >> 4) + t — and the norm sums are k_cos's own: identical bits.
// Blocks that hold no object (n <= 32: the third, n <= 16: the second) are skipped, wave-uniformly.
// ---------------------------------------------------------------------------------------------
constexpr int COSW_NB = 3;               // MFMA blocks per dimension a wave can hold: maps of up to 48 objects

__global__ void __launch_bounds__(256) k_cos_wave(DevParams D, int B, const ProbDesc* __restrict__ probs,
                                                  const double* __restrict__ feats, double* __restrict__ cosPool)
{
    const int b = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (b >= B) return;
    const ProbDesc pd = probs[b];
    if (pd.n1 <= 0 || pd.n2 <= 0) return;
    const int lane = threadIdx.x & 63;
    const int Fc = D.p.cos_feature_dim, coff = D.p.point_dim + D.p.ratio_feature_dim;
    const int lr = lane & 15, kq = lane >> 4;
    const int nbi = uni_i((pd.n1 + 15) >> 4), nbj = uni_i((pd.n2 + 15) >> 4);      // blocks in use per dimension (<= COSW_NB)
    const double* fa[COSW_NB]; const double* fb[COSW_NB]; bool va[COSW_NB], vb[COSW_NB];
#pragma unroll
    for (int h = 0; h < COSW_NB; ++h) {
        const int ia = 16 * h + lr, jb = 16 * h + lr;
        va[h] = ia < pd.n1; vb[h] = jb < pd.n2;
        fa[h] = feats + (pd.off1 + (va[h] ? ia : 0)) * D.F + coff + 4 * kq;
        fb[h] = feats + (pd.off2 + (vb[h] ? jb : 0)) * D.F + coff + 4 * kq;
    }
    double4_t acc[COSW_NB][COSW_NB];
#pragma unroll
    for (int x = 0; x < COSW_NB; ++x)
#pragma unroll
        for (int y = 0; y < COSW_NB; ++y) acc[x][y] = double4_t{0.0, 0.0, 0.0, 0.0};
    double sa[COSW_NB], sb[COSW_NB];
#pragma unroll
    for (int h = 0; h < COSW_NB; ++h) { sa[h] = 0.0; sb[h] = 0.0; }
    // the loads of chunk k0 + 16 are in flight while chunk k0 is multiplied (two register sets; all loads unconditional —
    // clamped to the last full chunk — so that the compiler waits with a count, not for an empty queue)
    int k0 = 0;
    const int nfull = Fc >> 4;                       // full chunks of 16
    d4u_t a[COSW_NB], bq[COSW_NB], a2[COSW_NB], b2[COSW_NB];
    auto fetch = [&](d4u_t (&ra)[COSW_NB], d4u_t (&rb)[COSW_NB], int kk) {
#pragma unroll
        for (int h = 0; h < COSW_NB; ++h) {
            if (h < nbi) ra[h] = *reinterpret_cast<const d4u_t*>(fa[h] + kk); else ra[h] = d4u_t{{0.0, 0.0, 0.0, 0.0}};
            if (h < nbj) rb[h] = *reinterpret_cast<const d4u_t*>(fb[h] + kk); else rb[h] = d4u_t{{0.0, 0.0, 0.0, 0.0}};
        }
    };
    auto multiply = [&](const d4u_t (&ra)[COSW_NB], const d4u_t (&rb)[COSW_NB]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int h = 0; h < COSW_NB; ++h) { sa[h] = fma(ra[h].v[t], ra[h].v[t], sa[h]); sb[h] = fma(rb[h].v[t], rb[h].v[t], sb[h]); }
#pragma unroll
            for (int x = 0; x < COSW_NB; ++x)
#pragma unroll
                for (int y = 0; y < COSW_NB; ++y)
                    if (x < nbi && y < nbj) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[x] ? ra[x].v[t] : 0.0, vb[y] ? rb[y].v[t] : 0.0, acc[x][y], 0, 0, 0);
        }
    };
    if (nfull > 0) {
        fetch(a, bq, 0);
        for (int c = 0; c < nfull; c += 2) {
            fetch(a2, b2, 16 * min(c + 1, nfull - 1));
            multiply(a, bq);
            if (c + 1 < nfull) {
                fetch(a, bq, 16 * min(c + 2, nfull - 1));
                multiply(a2, b2);
            }
        }
        k0 = 16 * nfull;
    }
    if (k0 < Fc) {                                   // ragged tail of the descriptor (< 16 elements)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kk = k0 + 4 * kq + t;
            const bool vk = kk < Fc;
            double av[COSW_NB], bv[COSW_NB];
#pragma unroll
            for (int h = 0; h < COSW_NB; ++h) {
                av[h] = (h < nbi && va[h] && vk) ? fa[h][k0 + t] : 0.0;
                bv[h] = (h < nbj && vb[h] && vk) ? fb[h][k0 + t] : 0.0;
                sa[h] = fma(av[h], av[h], sa[h]); sb[h] = fma(bv[h], bv[h], sb[h]);
            }
#pragma unroll
            for (int x = 0; x < COSW_NB; ++x)
#pragma unroll
                for (int y = 0; y < COSW_NB; ++y)
                    if (x < nbi && y < nbj) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
        }
    }
#pragma unroll
    for (int h = 0; h < COSW_NB; ++h) {              // every lane (lr, *) ends with the norm of row 16h + lr
        sa[h] += __shfl_xor(sa[h], 16); sa[h] += __shfl_xor(sa[h], 32);
        sb[h] += __shfl_xor(sb[h], 16); sb[h] += __shfl_xor(sb[h], 32);
        sa[h] = sqrt(sa[h]); sb[h] = sqrt(sb[h]);
    }
#pragma unroll
    for (int y = 0; y < COSW_NB; ++y) {
        const int col = 16 * y + lr;
        const double nb = sb[y];
#pragma unroll
        for (int x = 0; x < COSW_NB; ++x)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * x + kq + 4 * r;
                const double na = __shfl(sa[x], kq + 4 * r);       // norm of row 16x + (kq + 4r): held by lanes with lr == kq + 4r
                if (row < pd.n1 && col < pd.n2)
                    cosPool[pd.cosOff + (int64_t)row * pd.n2 + col] = D.pruned ? acc[x][y][r] : ((na > 0.0 && nb > 0.0) ? acc[x][y][r] / (na * nb) : 0.0);
            }
    }
}

// ---------------------------------------------------------------------------------------------
// k_cos_block: the cosine matrices of a FEW problems (a serial caller's one pair at a time) — maps of any size: a single pair of 200-object
// maps is 169 blocks on 169 waves, 6 us where the tile kernel's sixteen workgroups, two stages of loads in flight, take 29.  One wave alone walks a demo-size problem's
// 48 chunks x 36 matrix instructions in 68 us — the whole device idle beside it; here a wave takes ONE 16 x 16 block of the
// cosine matrix (up to nine waves per problem): four matrix instructions per chunk, eight chunks of loads in flight (a ring of
// 32-byte loads, refilled as it is consumed).  Every output element sees k_cos_wave's own contraction order — chunks of 16
// ascending, step t of a chunk contracts k = k0 + 4 * (lane >> 4) + t — and the norm sums are formed the same way: identical bits.
// ---------------------------------------------------------------------------------------------
constexpr int COSB_DEPTH = 8;

__global__ void __launch_bounds__(256) k_cos_block(DevParams D, int B, int nbx, int nby /* blocks per dimension of the largest problem of the call */,
                                                   const ProbDesc* __restrict__ probs,
                                                   const double* __restrict__ feats, double* __restrict__ cosPool)
{
    const int wid = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const int per = nbx * nby;
    const int b = uni_i(wid / per);
    if (b >= B) return;
    const int blk = uni_i(wid - b * per), xs = blk / nby, ys = blk - xs * nby;
    const ProbDesc pd = probs[b];
    if (16 * xs >= pd.n1 || 16 * ys >= pd.n2) return;
    const int lane = threadIdx.x & 63;
    const int Fc = D.p.cos_feature_dim, coff = D.p.point_dim + D.p.ratio_feature_dim;
    const int lr = lane & 15, kq = lane >> 4;
    const int ia = 16 * xs + lr, jb = 16 * ys + lr;
    const bool va = ia < pd.n1, vb = jb < pd.n2;
    const double* fa = feats + (pd.off1 + (va ? ia : 0)) * D.F + coff + 4 * kq;
    const double* fb = feats + (pd.off2 + (vb ? jb : 0)) * D.F + coff + 4 * kq;
    double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
    double sa = 0.0, sb = 0.0;
    const int nfull = Fc >> 4;
    if (nfull > 0) {
        d4u_t ra[COSB_DEPTH], rb[COSB_DEPTH];
#pragma unroll
        for (int t = 0; t < COSB_DEPTH; ++t) {
            const int kk = 16 * min(t, nfull - 1);
            ra[t] = *reinterpret_cast<const d4u_t*>(fa + kk); rb[t] = *reinterpret_cast<const d4u_t*>(fb + kk);
        }
        for (int c0 = 0; c0 < nfull; c0 += COSB_DEPTH) {
#pragma unroll
            for (int t = 0; t < COSB_DEPTH; ++t) {
                const d4u_t a = ra[t], q = rb[t];
                const int kn = 16 * min(c0 + t + COSB_DEPTH, nfull - 1);
                ra[t] = *reinterpret_cast<const d4u_t*>(fa + kn); rb[t] = *reinterpret_cast<const d4u_t*>(fb + kn);
                if (c0 + t < nfull) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        sa = fma(a.v[e], a.v[e], sa); sb = fma(q.v[e], q.v[e], sb);
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? a.v[e] : 0.0, vb ? q.v[e] : 0.0, acc, 0, 0, 0);
                    }
                }
            }
        }
    }
    const int k0 = 16 * nfull;
    if (k0 < Fc) {                                   // ragged tail of the descriptor (< 16 elements)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kk = k0 + 4 * kq + t;
            const bool vk = kk < Fc;
            const double av = (va && vk) ? fa[k0 + t] : 0.0, bv = (vb && vk) ? fb[k0 + t] : 0.0;
            sa = fma(av, av, sa); sb = fma(bv, bv, sb);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
    }
    sa += __shfl_xor(sa, 16); sa += __shfl_xor(sa, 32);
    sb += __shfl_xor(sb, 16); sb += __shfl_xor(sb, 32);
    sa = sqrt(sa); sb = sqrt(sb);
    const int col = 16 * ys + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * xs + kq + 4 * r;
        const double na = __shfl(sa, kq + 4 * r);
        if (row < pd.n1 && col < pd.n2)
            cosPool[pd.cosOff + (int64_t)row * pd.n2 + col] = D.pruned ? acc[r] : ((na > 0.0 && sb > 0.0) ? acc[r] / (na * sb) : 0.0);
    }
}

// ---------------------------------------------------------------------------------------------
// k_cos_tile: the same products, operands staged through LDS.  A workgroup (4 waves) owns an output tile of up to 64x64,
// wave (wy, wx) the 2x2 MFMA blocks of its quarter.  Per stage of KC descriptor elements the 256 threads copy the tile's
// row pieces of KC doubles from global memory to LDS with 16-byte loads whose lanes run ALONG a row (SEGS lanes cover one
// row piece contiguously): every cache line that is touched is used completely, and a row is fetched once per workgroup
// instead of once per wave — 256 bytes of loads per MFMA instead of 512.  Why that matters (rocprofv3 round 3, config 3):
// the matrix pipe of k_cos is busy 42 % of the time; a load takes ~1.6 us under this load, so keeping the pipe fed takes
// (bytes per MFMA) x (MFMA rate) x 1.6 us ~ 100 KB in flight per compute unit, and a wave of k_cos has nothing in flight
// while it multiplies.  Here the loads of stages s + 1 and s + 2 are in flight while stage s is multiplied (two register
// sets, two LDS stages, one barrier per stage).
// Tiles are BALANCED: a dimension of nb 16-row blocks is cut into ceil(nb / 4) tiles of nb / tiles blocks, rounded either
// way (13 blocks: 3 + 3 + 3 + 4, not 4 + 4 + 4 + 1) — a workgroup with one block column would wait for its loads 32 times
// to issue a quarter of the MFMAs while it holds a quarter of the compute unit's registers.
// The contraction order of every output element is k_cos' own — chunks of 16 ascending, MFMA t of a chunk contracts
// k = k0 + 4 * (lane >> 4) + t —, so are the norm sums: identical bits.
// ---------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(8))) d2u_t { double v[2]; };      // 8-byte aligned 16-byte load

__device__ __forceinline__ int cos_tiles(int n) { return (((n + 15) >> 4) + 3) >> 2; }            // tiles along a dimension of n rows
constexpr int COS_KC = 16;                   // descriptor elements per stage of k_cos_tile

__global__ void __launch_bounds__(256) k_cos_tile(DevParams D, int B, int G /* workgroups (tiles) per problem */,
                                                  const ProbDesc* __restrict__ probs,
                                                  const double* __restrict__ feats,
                                                  double* __restrict__ cosPool)
{
    constexpr int KC = COS_KC;
    constexpr int PITCH = KC * 8 + 16;           // bytes per staged row piece (the 16 spread the rows over the banks)
    constexpr int SEGS = KC / 2;                 // 16-byte segments per row piece
    constexpr int RPI = 256 / SEGS;              // rows per load instruction of the workgroup
    constexpr int NLD = 128 / RPI;               // load instructions per stage and thread (first half: A rows, second half: B rows)
    constexpr int STAGE = 128 * PITCH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 2 stages x (64 A rows + 64 B rows) x PITCH
    // (the grid is rounded up to whole groups of eight problems: slots behind the last tile are passed by)
    const int xcd = blockIdx.x & 7, nSlots = G * ((B + 7) >> 3);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int slot = blockIdx.x >> 3; slot < nSlots; slot += gridDim.x >> 3) {
    const int b = (slot / G) * 8 + xcd;          // all tiles of a problem on one XCD (k_cos)
    if (b >= B) continue;
    const ProbDesc pd = probs[b];
    const int ti_n = cos_tiles(pd.n1), tj_n = cos_tiles(pd.n2);
    const int tile = slot % G;
    if (tile >= ti_n * tj_n) continue;
    const int ti = tile / tj_n, tj = tile - ti * tj_n;
    const int nbi = (pd.n1 + 15) >> 4, nbj = (pd.n2 + 15) >> 4;
    const int bi0 = ti * nbi / ti_n, bj0 = tj * nbj / tj_n;                    // first block of the tile
    const int nbx = (ti + 1) * nbi / ti_n - bi0, nby = (tj + 1) * nbj / tj_n - bj0;   // blocks of the tile: 1..4
    const int i0 = bi0 * 16, j0 = bj0 * 16;
    const int iEnd = min(pd.n1, i0 + 16 * nbx), jEnd = min(pd.n2, j0 + 16 * nby);    // rows / columns of the tile
    const int Fc = D.p.cos_feature_dim, coff = D.p.point_dim + D.p.ratio_feature_dim;
    const int lr = lane & 15, kq = lane >> 4;
    // A wave takes ONE block row of the tile (all its nby blocks) or, when the tile has more block columns than rows, one block
    // column: a 3x3 tile keeps three waves busy with 3 blocks each, 3x4 and 4x3 tiles all four — dealt as 2x2 quarters they
    // were 4 + 2 + 2 + 1 and the workgroup as slow as a full tile (tools/ubench/mfma_tiles.hip: 213 us against the 169 of a
    // perfect deal for config 3).  Which wave takes which row rotates with the tile: a wave index is a SIMD.
    // A tile of at most 2x2 blocks (maps of up to 32 objects: the reference's demo scale) gives every wave ONE block.
    const bool oneBlock = nbx <= 2 && nby <= 2;
    const bool byRows = oneBlock || nbx >= nby;
    const int wsr = (w + tile) & 3;
    const int ws = oneBlock ? (wsr >> 1) : wsr;                  // the wave's block row (byRows) or block column
    const int m0 = oneBlock ? (wsr & 1) : 0;                     // first of its blocks across
    const int nMin = uni_i(oneBlock ? ((ws < nbx && m0 < nby) ? 1 : 0)
                                    : (ws < (byRows ? nbx : nby) ? (byRows ? nby : nbx) : 0));      // blocks of this wave: 0..4

    // the thread's share of a stage
    const int seg = tid % SEGS, row0 = tid / SEGS;
    const double* gp[NLD]; bool gv[NLD];
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
        const int r = (q * RPI + row0) & 63;
        const bool isA = q < NLD / 2;
        const int gr = (isA ? i0 : j0) + r;
        gv[q] = gr < (isA ? iEnd : jEnd);
        gp[q] = feats + ((isA ? pd.off1 : pd.off2) + (gv[q] ? gr : 0)) * D.F + coff + 2 * seg;
    }
    // (no control flow around the loads of the main loop: the compiler's wait-count pass then lets two stages fly)
    auto gload = [&](dbl2_t (&stg)[NLD], int k0) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const d2u_t t = *reinterpret_cast<const d2u_t*>(gp[q] + k0);
            stg[q] = dbl2_t{t.v[0], t.v[1]};
        }
    };
    auto gload_ragged = [&](dbl2_t (&stg)[NLD], int k0) {      // last stage of a descriptor that is no multiple of KC: element by element
        const int k = k0 + 2 * seg;
#pragma unroll
        for (int q = 0; q < NLD; ++q) stg[q] = dbl2_t{k < Fc ? gp[q][k0] : 0.0, k + 1 < Fc ? gp[q][k0 + 1] : 0.0};
    };
    auto lstore = [&](const dbl2_t (&stg)[NLD], int buf) {
#pragma unroll
        for (int q = 0; q < NLD; ++q)                // rows behind the tile: zeros
            *reinterpret_cast<dbl2_t*>(smem + buf * STAGE + (q * RPI + row0) * PITCH + seg * 16) = gv[q] ? stg[q] : dbl2_t{0.0, 0.0};
    };

    double4_t acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = double4_t{0.0, 0.0, 0.0, 0.0};
    double sMaj = 0.0, sMin[4] = {0.0, 0.0, 0.0, 0.0};
    // LDS offsets of the lane's 32-byte pieces: A rows are stage rows 0..63, B rows 64..127
    const int offMaj = ((byRows ? 0 : 64) + 16 * ws + lr) * PITCH + 32 * kq;
    const int offMin = ((byRows ? 64 : 0) + 16 * m0 + lr) * PITCH + 32 * kq;

    auto compute = [&](int s) {
        const unsigned char* base = smem + (s & 1) * STAGE;
        if (nMin > 0) {
#pragma unroll
            for (int kc = 0; kc < KC; kc += 16) {
                if (s * KC + kc < Fc) {
                    // block by block (the four MFMAs of a block depend on each other through the accumulator: forwarded in the
                    // matrix pipe; every accumulator still sees t = 0..3 of chunk after chunk — its own order is unchanged):
                    // 16 operand registers instead of 40, and the reads of the next block fly behind the MFMAs of this one
                    double mj[4];
                    {
                        const dbl2_t v0 = *reinterpret_cast<const dbl2_t*>(base + offMaj + kc * 8);
                        const dbl2_t v1 = *reinterpret_cast<const dbl2_t*>(base + offMaj + kc * 8 + 16);
                        mj[0] = v0.x; mj[1] = v0.y; mj[2] = v1.x; mj[3] = v1.y;
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) sMaj = fma(mj[t], mj[t], sMaj);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        if (m < nMin) {
                            const dbl2_t v0 = *reinterpret_cast<const dbl2_t*>(base + offMin + 16 * m * PITCH + kc * 8);
                            const dbl2_t v1 = *reinterpret_cast<const dbl2_t*>(base + offMin + 16 * m * PITCH + kc * 8 + 16);
                            const double mn[4] = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                sMin[m] = fma(mn[t], mn[t], sMin[m]);
                                // a column wave multiplies B A^T: the TRANSPOSED block — the same products, summed in the same k order
                                acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(mj[t], mn[t], acc[m], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
    };

    // stage s is multiplied while the loads of stages s + 1 (register set of the other parity) and s + 2 (this parity's) fly
    // (a third set — three stages in flight — measured 3 % slower at config 3 and at the demo scale)
    // (every load of the loop is UNCONDITIONAL — beyond the last stage it fetches that stage again: a load inside an `if`
    // makes the compiler's wait-count pass assume the shorter queue at the join and wait for everything in flight)
    const int SF = Fc / KC;                          // full stages; a ragged one may follow
    dbl2_t r0[NLD], r1[NLD];
    if (SF > 0) {
        gload(r0, 0);
        gload(r1, min(1, SF - 1) * KC);
        lstore(r0, 0);
        __syncthreads();
        for (int s = 0; s < SF; s += 2) {
            gload(r0, min(s + 2, SF - 1) * KC);
            compute(s);
            lstore(r1, 1);
            __syncthreads();
            gload(r1, min(s + 3, SF - 1) * KC);
            if (s + 1 < SF) compute(s + 1);
            lstore(r0, 0);
            __syncthreads();
        }
    }
    if (SF * KC < Fc) {                              // (every wave is behind the last barrier: both LDS stages are free)
        gload_ragged(r0, SF * KC);
        lstore(r0, SF & 1);
        __syncthreads();
        compute(SF);
    }
    // every lane (lr, *) ends with the norm of row lr of the block
    sMaj += __shfl_xor(sMaj, 16); sMaj += __shfl_xor(sMaj, 32); sMaj = sqrt(sMaj);
#pragma unroll
    for (int m = 0; m < 4; ++m) { sMin[m] += __shfl_xor(sMin[m], 16); sMin[m] += __shfl_xor(sMin[m], 32); sMin[m] = sqrt(sMin[m]); }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m < nMin) {                              // (the divisions run on the same f64 units as the MFMAs)
            // acc[m][r] of lane (lr, kq) is element (kq + 4r, lr) of (own block) x (block m across)^T
            const double nLr = sMin[m];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double nOwn = __shfl(sMaj, kq + 4 * r);      // norm of row (kq + 4r) of the own block: held by lanes with lr == kq + 4r
                const int row = byRows ? i0 + 16 * ws + kq + 4 * r : i0 + 16 * (m0 + m) + lr;
                const int col = byRows ? j0 + 16 * (m0 + m) + lr : j0 + 16 * ws + kq + 4 * r;
                const double na = byRows ? nOwn : nLr, nb = byRows ? nLr : nOwn;
                if (row < iEnd && col < jEnd)
                    cosPool[pd.cosOff + (int64_t)row * pd.n2 + col] = D.pruned ? acc[m][r] : ((na > 0.0 && nb > 0.0) ? acc[m][r] / (na * nb) : 0.0);
            }
        }
    }
    __syncthreads();                                 // the next tile's first stage overwrites LDS stage 0
    }
}

// ---------------------------------------------------------------------------------------------
// k_cos_deal<T>: the cosine matrices of a BATCH of mid-size maps (config 3: 256 pairs of 200 x 200 objects).  k_cos_tile's tiles
// are at most 4 x 4 blocks and a wave owns one block row of its tile: at 13 blocks per dimension (200 objects) the balanced
// tiling is 3 + 3 + 3 + 4, nine of the sixteen tiles are 3 x 3 and leave one wave of four without a block — the matrix pipe
// cannot be busier than 169 / 256 of the time (measured: 0.5).  Here a tile is up to T x T blocks (T = 5; 13 blocks: 5 + 4 + 4)
// and its BLOCKS are dealt to the four waves as equal runs of the row-major block list — 25, 20, 16 blocks: 6-7, 5, 4 per wave,
// 169 of 172 block slots used —; a wave holds up to 7 accumulators, reads the operands of its next block from LDS in front of
// the MFMAs of the current one, and a staged row feeds 4-5 blocks instead of 3-4.  LDS: two stages of (80 + 80) row pieces of
// 16 doubles = 46 KB, 153 registers: three workgroups per compute unit.
// Measured alone on config 3's shape (tools/ubench/cos_time.hip, one box): k_cos_tile 361 us, T = 7 (two workgroups per CU, 13
// accumulators) 344, T = 6 362, T = 5 321, T = 4 365; in the batch pipeline (rocprofv3) 322 -> 290 us.  The same tool strips parts
// of the kernel: without global loads, LDS stores, barriers and norms the T = 5 loop takes 208 us (the matrix pipe's own time for
// this deal), and every part that is put back costs 20-80 us, sub-additively — because the kernel is POWER-bound: a probe wave
// per XCD (clock64 against wall_clock64) sees the shader clock fall from 2.4 GHz (idle) to 2.1-2.2 GHz under the stripped loop
// and to 1.7-2.0 GHz under the complete kernel (k_cos_tile alike).  What makes this kernel faster is less work per MFMA.
// The launcher picks it when the batch has at least two workgroups per compute unit of such tiles; a single alignment keeps
// k_cos_tile's sixteen small tiles (latency).
// Bits: a block's MFMA sequence is k_cos's own (chunks of 16 ascending, MFMA t of a chunk contracts k = k0 + 4 (lane >> 4) + t);
// the norms are summed by a separate pass over the staged rows in the order of k_cos_tile's (lane (lr, kq): its k's ascending,
// then the two cross-quarter adds) and handed over through LDS.  Identical bits.
// ---------------------------------------------------------------------------------------------
constexpr int COSD_PITCH = 16 * 8 + 16;          // bytes per staged row piece (k_cos_tile's)
template <int T> struct CosDeal {                // T: blocks per tile and dimension
    static constexpr int ROWS = 2 * 16 * T;      // staged row pieces: A rows 0..16T-1, B rows 16T..32T-1
    static constexpr int STAGE = ROWS * COSD_PITCH;
    static constexpr int MAXB = (T * T + 3) / 4; // blocks of a wave
    static constexpr int LDS = 2 * STAGE + ROWS * 8;                    // two stages + the norms
    static constexpr int WAVES = T <= 5 ? 3 : 2; // waves per SIMD the registers are capped for (workgroups per compute unit)
    __device__ __host__ static int tiles(int n) { return (((n + 15) >> 4) + T - 1) / T; }
};

template <int T, int DBG /* 0; tools/ubench/cos_time.hip strips parts of the kernel to time the rest: 1 no loads in the loop, 2 no LDS stores / barriers, 4 no MFMAs, 8 no norms */>
__global__ void __launch_bounds__(256, CosDeal<T>::WAVES) k_cos_deal(DevParams D, int B, int G /* workgroups (tiles) per problem */,
                                                     const ProbDesc* __restrict__ probs,
                                                     const double* __restrict__ feats,
                                                     double* __restrict__ cosPool,
                                                     const int32_t* __restrict__ only /* NULL, or [B]: problems with a 0 are skipped (behind k_cos_sel) */)
{
    using CD = CosDeal<T>;
    constexpr int KC = 16, PITCH = COSD_PITCH, SEGS = KC / 2, RPI = 256 / SEGS, NLD = CD::ROWS / RPI, STAGE = CD::STAGE, MAXB = CD::MAXB;
    static_assert(NLD * RPI == CD::ROWS, "the workgroup's loads cover a stage exactly");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* nrm = reinterpret_cast<double*>(smem + 2 * STAGE);          // norm of staged row r
    // eight problems or more: all tiles of a problem on one XCD (they share its rows); fewer (grid = B * G): tiles over all XCDs
    const int xcd = blockIdx.x & 7, slot = B >= 8 ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = uni_i(tid >> 6);
    const int b = B >= 8 ? (slot / G) * 8 + xcd : slot / G;
    if (b >= B) return;
    if (only && !only[b]) return;
    const ProbDesc pd = probs[b];
    const int ti_n = CD::tiles(pd.n1), tj_n = CD::tiles(pd.n2);
    const int tile = slot % G;
    if (tile >= ti_n * tj_n) return;
    const int ti = tile / tj_n, tj = tile - ti * tj_n;
    const int nbi = (pd.n1 + 15) >> 4, nbj = (pd.n2 + 15) >> 4;
    const int bi0 = ti * nbi / ti_n, bj0 = tj * nbj / tj_n;                    // first block of the tile (balanced cut)
    const int nbx = uni_i((ti + 1) * nbi / ti_n - bi0), nby = uni_i((tj + 1) * nbj / tj_n - bj0);   // blocks of the tile: 1..T
    const int i0 = bi0 * 16, j0 = bj0 * 16;
    const int iEnd = min(pd.n1, i0 + 16 * nbx), jEnd = min(pd.n2, j0 + 16 * nby);
    const int Fc = D.p.cos_feature_dim, coff = D.p.point_dim + D.p.ratio_feature_dim;
    const int lr = lane & 15, kq = lane >> 4;
    // the wave's run of the tile's row-major block list (which wave takes which run rotates with the tile: a wave index is a SIMD)
    const int wsr = (w + tile) & 3, nblk = nbx * nby;
    const int e0 = uni_i(wsr * nblk / 4), cnt = uni_i((wsr + 1) * nblk / 4 - e0);        // <= MAXB
    const int lanePart = lr * PITCH + 32 * kq;
    int offA[MAXB], offB[MAXB]; bool newRow[MAXB];
#pragma unroll
    for (int m = 0; m < MAXB; ++m) {
        const int e = min(e0 + m, nblk - 1), bx = e / nby, by = e - bx * nby;
        offA[m] = uni_i(16 * bx * PITCH); offB[m] = uni_i((16 * T + 16 * by) * PITCH);
        newRow[m] = uni_i((by == 0 && e0 + m < nblk) ? 1 : 0) != 0;
    }

    // the thread's share of a stage
    const int seg = tid % SEGS, row0 = tid / SEGS;
    const double* gp[NLD]; bool gv[NLD];
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
        const int r = q * RPI + row0;
        const bool isA = r < 16 * T;
        const int gr = isA ? i0 + r : j0 + r - 16 * T;
        gv[q] = gr < (isA ? iEnd : jEnd);
        gp[q] = feats + ((isA ? pd.off1 : pd.off2) + (gv[q] ? gr : 0)) * D.F + coff + 2 * seg;
    }
    // (no control flow around the loads of the main loop — k_cos_tile)
    auto gload = [&](dbl2_t (&stg)[NLD], int k0) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const d2u_t t = *reinterpret_cast<const d2u_t*>(gp[q] + k0);
            stg[q] = dbl2_t{t.v[0], t.v[1]};
        }
    };
    auto gload_ragged = [&](dbl2_t (&stg)[NLD], int k0) {      // last stage of a descriptor that is no multiple of 16: element by element
        const int k = k0 + 2 * seg;
#pragma unroll
        for (int q = 0; q < NLD; ++q) stg[q] = dbl2_t{k < Fc ? gp[q][k0] : 0.0, k + 1 < Fc ? gp[q][k0 + 1] : 0.0};
    };
    auto lstore = [&](const dbl2_t (&stg)[NLD], int buf) {
#pragma unroll
        for (int q = 0; q < NLD; ++q)                // rows behind the tile: zeros
            *reinterpret_cast<dbl2_t*>(smem + buf * STAGE + (q * RPI + row0) * PITCH + seg * 16) = gv[q] ? stg[q] : dbl2_t{0.0, 0.0};
    };

    double4_t acc[MAXB];
#pragma unroll
    for (int m = 0; m < MAXB; ++m) acc[m] = double4_t{0.0, 0.0, 0.0, 0.0};
    // norms: wave w sums the 16-row blocks w, w + 4, w + 8, ... of the stage's 2 T (those that hold rows of the tile)
    constexpr int NNB = (2 * T + 3) / 4;
    double sN[NNB]; bool nOn[NNB];
#pragma unroll
    for (int h = 0; h < NNB; ++h) {
        const int hb = w + 4 * h;
        sN[h] = 0.0;
        nOn[h] = uni_i((hb < T ? hb < nbx : (hb < 2 * T && hb - T < nby)) ? 1 : 0) != 0;
    }

    // Operands of block m + 1 are read from LDS BEFORE the four MFMAs of block m are issued (two register sets): the wave never
    // waits for LDS with an idle matrix pipe behind it.  The read behind the last block fetches that block again (offsets clamped).
    // The norms' f64 FMAs (the units the f64 MFMAs occupy) come as one burst behind the stage's MFMAs: measured equal to spreading
    // them between the blocks with their operands read ahead (tools/ubench/cos_time.hip).  A norm's own order — its lane's k
    // ascending — is k_cos_tile's.
    auto norm_sum = [&](int h, const dbl2_t& v0, const dbl2_t& v1) {
        sN[h] = fma(v0.x, v0.x, sN[h]); sN[h] = fma(v0.y, v0.y, sN[h]); sN[h] = fma(v1.x, v1.x, sN[h]); sN[h] = fma(v1.y, v1.y, sN[h]);
    };
    auto compute = [&](int s) {
        const unsigned char* base = smem + (s & 1) * STAGE + lanePart;
        dbl2_t a0, a1, b0, b1;
        a0 = *reinterpret_cast<const dbl2_t*>(base + offA[0]); a1 = *reinterpret_cast<const dbl2_t*>(base + offA[0] + 16);
        b0 = *reinterpret_cast<const dbl2_t*>(base + offB[0]); b1 = *reinterpret_cast<const dbl2_t*>(base + offB[0] + 16);
#pragma unroll
        for (int m = 0; m < MAXB; ++m) {
            if (m < cnt) {
                dbl2_t na0 = a0, na1 = a1, nb0 = b0, nb1 = b1;
                if (m + 1 < MAXB) {
                    nb0 = *reinterpret_cast<const dbl2_t*>(base + offB[m + 1]); nb1 = *reinterpret_cast<const dbl2_t*>(base + offB[m + 1] + 16);
                    if (newRow[m + 1]) {                 // the next block starts a block row: its A operand
                        na0 = *reinterpret_cast<const dbl2_t*>(base + offA[m + 1]); na1 = *reinterpret_cast<const dbl2_t*>(base + offA[m + 1] + 16);
                    }
                }
                if (!(DBG & 4)) {
                    acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b0.x, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b0.y, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b1.x, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b1.y, acc[m], 0, 0, 0);
                } else { acc[m][0] += a0.x + b0.x; acc[m][1] += a0.y + b0.y; acc[m][2] += a1.x + b1.x; acc[m][3] += a1.y + b1.y; }
                a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
            }
        }
        if (!(DBG & 8)) {
#pragma unroll
            for (int h = 0; h < NNB; ++h)
                if (nOn[h]) {
                    const dbl2_t v0 = *reinterpret_cast<const dbl2_t*>(base + 16 * (w + 4 * h) * PITCH);
                    const dbl2_t v1 = *reinterpret_cast<const dbl2_t*>(base + 16 * (w + 4 * h) * PITCH + 16);
                    norm_sum(h, v0, v1);
                }
        }
    };

    // stage s is multiplied while the loads of stages s + 1 and s + 2 fly (k_cos_tile's loop)
    const int SF = Fc / KC;
    dbl2_t r0[NLD], r1[NLD];
    if (SF > 0) {
        gload(r0, 0);
        gload(r1, min(1, SF - 1) * KC);
        lstore(r0, 0);
        __syncthreads();
        for (int s = 0; s < SF; s += 2) {
            if (!(DBG & 1)) gload(r0, min(s + 2, SF - 1) * KC);
            compute(s);
            if (!(DBG & 2)) { lstore(r1, 1); __syncthreads(); }
            if (!(DBG & 1)) gload(r1, min(s + 3, SF - 1) * KC);
            if (s + 1 < SF) compute(s + 1);
            if (!(DBG & 2)) { lstore(r0, 0); __syncthreads(); }
        }
    }
    if (SF * KC < Fc) {                              // (every wave is behind the last barrier: both LDS stages are free)
        gload_ragged(r0, SF * KC);
        lstore(r0, SF & 1);
        __syncthreads();
        compute(SF);
    }
#pragma unroll
    for (int h = 0; h < NNB; ++h) {
        double v = sN[h];
        v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
        if (nOn[h] && kq == 0) nrm[16 * (w + 4 * h) + lr] = sqrt(v);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MAXB; ++m) {
        if (m < cnt) {
            // acc[m][r] of lane (lr, kq) is element (kq + 4r, lr) of (block row bx) x (block column by)^T
            const int e = e0 + m, bx = e / nby, by = e - bx * nby;
            const int col = j0 + 16 * by + lr;
            const double nb = nrm[16 * T + 16 * by + lr];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + 16 * bx + kq + 4 * r;
                const double na = nrm[16 * bx + kq + 4 * r];
                if (row < iEnd && col < jEnd)
                    cosPool[pd.cosOff + (int64_t)row * pd.n2 + col] = D.pruned ? acc[m][r] : ((na > 0.0 && nb > 0.0) ? acc[m][r] / (na * nb) : 0.0);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_cos_sel (round 6): the cosine matrices of a batch whose cosines are only used behind the gate cos > cosine_min
// (single_score(): an association with (cos - cosine_min) / (cosine_max - cosine_min) <= 0 scores 0 whatever its cosine is).
// k_cos_deal computes all n1 x n2 cosines in f64 on the matrix core and is POWER-bound (295 us at config 3); ~95 % of its
// products are thrown away by the gate.  Here one workgroup of 16 waves takes a problem:
//   pass 1  approximate cosines of all pairs: rows converted to bf16 on the way into LDS (f64 -> f32 -> bf16, each conversion ROUND TO
//           NEAREST EVEN: a unit roundoff of 2^-8 for bf16.  tests/_bf16_screen.py models exactly this conversion and the device's
//           screen is held to the model within the accumulation term below; a truncating conversion would keep the bound — it only
//           shrinks: a uniform 2^-8 that the rows' own norms divide out, plus a symmetric 2^-8 — but not that agreement),
//           v_mfma_f32_16x16x32_bf16 (1/32 of the f64 MFMA's matrix-pipe time), divided by the bf16 rows' OWN norms (the diagonals of the
//           same bf16 products, accumulated in f32) — not by the exact f64 norms;
//   select  pair (i, j) is a CANDIDATE unless approx < cosine_min - delta.  The screen is the exact cosine of the rounded rows a^, b^;
//           each rounding turns a row by an angle of at most asin(2^-8 (1 + 2^-24)), so |cos(a^, b^) - cos(a, b)| <= ~2 * 2^-8 = 2^-7,
//           plus ~3 Fc 2^-24 (the f32 accumulation of the product and of the two norms, any order, truncating or not: 2^-13 at
//           Fc = 512) — about 0.0079 for rows whose norm lies in [2^-40, 2^40] (no element over- or underflows in bf16 / f32 beyond 2^-86 of the product of
//           the norms); rows with any other non-zero norm (huge, tiny, inf, NaN) make all their pairs candidates.  delta = 2^-6: a
//           margin of 2x the bound.
//   pass 2  the candidates' dot products in f64 with k_cos_deal's own contraction order (oracle dot_fixed(): per chunk of 16, t = 0..3
//           outer, g = 0..3 inner, k = k0 + 4 g + t, ONE fma chain), rows staged through LDS chunk by chunk, candidates sorted by i so
//           that the lanes of a wave read few distinct a rows (LDS broadcast); the exact norms summed from the same staged chunks in the
//           oracle's stated order (four chains, (s0 + s1) + (s2 + s3)); cos = dot / (na * nb) as everywhere.
// A non-candidate's entry of the pool holds the APPROXIMATE cosine (< cosine_min - delta + 2^-7 < cosine_min, and so is the exact one:
// both fail the gate alike).  Candidates' entries are bit-identical to k_cos_deal's.  A problem with more than CSEL_CAP candidates (or maps
// of more than 256 objects) is flagged in dense[] and left to k_cos_deal<., ., true>, which the launcher runs behind this kernel for the
// flagged problems only.  Never used for the pruned prefilter (raw products) / cosine_max <= cosine_min.  k_cos_sel itself serves
// roman_debug_cosine (ROMAN_COS_SEL=approx / gated); the batched path takes k_cos_live (below: the same passes, no cosine matrix).
// ---------------------------------------------------------------------------------------------
constexpr int CSEL_ROWS = 512;                   // staged rows: A rows [0, 16 nb1), B rows [16 nb1, 16 nb1 + 16 nb2)
constexpr int CSEL_MAXN = 256;                   // objects per map
constexpr int CSEL_CAP = 4096;                   // candidates per problem (config 3: ~2200 of 40000); four per thread in pass 2
constexpr int CSEL_NPT = CSEL_CAP / 1024;        // candidates per thread
constexpr int CSEL_P1 = 256 + 16;                // bytes per staged row of pass 1: 128 bf16 + pad
constexpr int CSEL_P2 = 128 + 16;                // bytes per staged row of pass 2: 16 doubles + pad
constexpr int CSEL_MP = 11;                    // blocks of the product per wave: problems of up to 176 blocks of 16 x 16 (200 x 200 objects: 169)
constexpr int CSEL_STAGE = CSEL_ROWS * CSEL_P1;  // pass 1: the tile; behind it: pass 2's chunk and the candidate lists
static_assert(CSEL_ROWS * CSEL_P2 + 2 * CSEL_CAP * 4 <= CSEL_STAGE, "pass 2 fits where the tile was");
constexpr int CSEL_LDS = CSEL_STAGE + CSEL_ROWS * 8 + 2 * 260 * 4;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(8))) d8u_t { double v[8]; };     // 8-byte aligned 64-byte load

__device__ __forceinline__ bool csel_unsafe(double n) { return !(n >= 0x1p-40 && n <= 0x1p40); }

// (a problem's live associations: the kind of solver its live count takes — k_live<1> and k_cos_live)
__device__ __forceinline__ int live_kind(const DevParams& D, int L)
{
    return (L <= D.stream_maxL && D.p.maxiniters >= 1 && D.p.maxlsiters >= 1) ? 0 : (D.allow_fallback ? 1 : 2);
}

// The body of k_cos_sel (LIVE = false: the cosine matrix) and of k_cos_live (LIVE = true: gate, single scores and the live pools of the
// problem; nothing in cosPool).  `lv` is only read with LIVE.
struct CselLive { ProbState* st; int32_t* lp; int32_t* li; int32_t* lj; double* ls; double* ld; double* lza; double* lzb; };

template <bool LIVE>
__device__ __forceinline__ void cos_sel_body(const DevParams& D, int B, const ProbDesc* __restrict__ probs, const double* __restrict__ feats,
                                             double* __restrict__ cosPool, int32_t* __restrict__ dense, double thr, const CselLive& lv)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* stage = smem;
    double* nrm = reinterpret_cast<double*>(smem + CSEL_STAGE);
    uint32_t* U = reinterpret_cast<uint32_t*>(smem + CSEL_ROWS * CSEL_P2);   // candidates as found: i | j << 16 (where the tile was: behind pass 2's chunk)
    uint32_t* S = U + CSEL_CAP;                                          // sorted by i
    int* hist = reinterpret_cast<int*>(nrm + CSEL_ROWS);                 // [0, 256): candidates of row i; [256]: all
    int* cur = hist + 260;
    const int b = blockIdx.x;
    if (b >= B) return;
    const ProbDesc pd = probs[b];
    const int tid = threadIdx.x, lane = tid & 63, w = uni_i(tid >> 6);
    const int n1 = pd.n1, n2 = pd.n2;
    auto publish = [&](int L) {                                          // (LIVE: what k_live<1> writes for the problem)
        if (LIVE && tid == 0) { lv.st[b].L = L; lv.st[b].nnzUpper = 0ull; lv.st[b].kind = live_kind(D, L); }
    };
#ifdef ROMAN_CSEL_TIMING
    unsigned long long tc_[5]; tc_[0] = __builtin_readcyclecounter();
#define CMARK(i_) tc_[i_] = __builtin_readcyclecounter()
#else
#define CMARK(i_) do { } while (0)
#endif
    if (n1 <= 0 || n2 <= 0) { if (tid == 0) dense[b] = 0; publish(0); return; }
    const int nb1 = (n1 + 15) >> 4, nb2 = (n2 + 15) >> 4, RB = 16 * nb1, nblk = nb1 * nb2, rowsTot = RB + 16 * nb2;
    if (n1 > CSEL_MAXN || n2 > CSEL_MAXN || nblk > 16 * CSEL_MP) { if (tid == 0) dense[b] = 1; return; }
    const int Fc = D.p.cos_feature_dim, coff = D.p.point_dim + D.p.ratio_feature_dim;
    if (tid < 260) hist[tid] = 0;
    const double* base1 = feats + pd.off1 * D.F + coff;
    const double* base2 = feats + pd.off2 * D.F + coff;
    // staged row R holds object R of map 1 (R < RB) or object R - RB of map 2; rows behind a map's last object: zeros

    // ---- pass 1 -------------------------------------------------------------------------------------------
    // loads: one wave instruction reads 128 consecutive elements — ONE KILOBYTE — of one row: lane l the elements k0 + 2 l, k0 + 2 l + 1.
    // (Pieces of 128 / 256 B of eight / four rows per instruction — what a tile of 16 / 32 elements of every row needs — ran this pass
    // at 127 / 115 us whatever the prefetch depth: 256 workgroups x 416 rows are 10^5 streams of short bursts for the DRAM.)  A tile is
    // 128 elements of every row as bf16 (rows x 272 B); wave w owns the rows w, w + 16, ...; four rows per register set, two sets, each
    // re-loaded as soon as it is staged — also across the tile's barrier and its MFMAs.
    // The screen's norms are the bf16 rows' own (the diagonals of the products of every block of 16 rows with itself: wave w the
    // blocks w, w + 16 — no f64 arithmetic in this pass): cos(a^, b^) against cos(a, b) — two angles of at most asin(2^-8) (see the bound above).
    constexpr int KT = 128, G1 = 4;
    const int nt = rowsTot >> 4;                                         // rows of a wave
    // No branch and no address arithmetic inside the stream of loads (a branch makes the compiler wait for ALL outstanding loads at its
    // join; the rows' addresses computed per load were 5800 scalar instructions per wave — the scalar unit busy 40 % of the pass): lane t
    // of the wave holds the address of the wave's row slot t — a slot behind the wave's last row, or a row behind its map's last object,
    // holds the last real one's (a cache hit; staged into a tile row whose products nobody reads: C[i][j] depends on rows i and j alone)
    // — and a slot's load takes it from there (v_readlane) as its scalar base.
    const int NG8 = ((nt + 2 * G1 - 1) / (2 * G1)) * 2;                  // groups of a tile, an even number
    const int NSF = Fc / KT;                                             // full tiles
    uint32_t slotLo, slotHi;
    {
        const int R = w + 16 * min(lane, nt - 1);
        const bool isA = R < RB;
        const int idx = min(isA ? R : R - RB, (isA ? n1 : n2) - 1);
        const uint64_t pa = reinterpret_cast<uint64_t>((isA ? base1 : base2) + (int64_t)idx * D.F);
        slotLo = (uint32_t)pa; slotHi = (uint32_t)(pa >> 32);
    }
    auto slot_ptr = [&](int t) -> const double* {                        // (wave-uniform)
        const uint64_t lo = (uint32_t)__builtin_amdgcn_readlane((int)slotLo, t), hi = (uint32_t)__builtin_amdgcn_readlane((int)slotHi, t);
        return reinterpret_cast<const double*>((hi << 32) | lo);
    };
    auto load_group = [&](dbl2_t (&x)[G1], int st, int g) {
        const int ko = st * KT + 2 * lane;
#pragma unroll
        for (int j = 0; j < G1; ++j) {
            const d2u_t tv = *reinterpret_cast<const d2u_t*>(slot_ptr(G1 * g + j) + ko);
            x[j] = dbl2_t{tv.v[0], tv.v[1]};
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto load_group_ragged = [&](dbl2_t (&x)[G1], int st, int g) {
        const int k = st * KT + 2 * lane;
#pragma unroll
        for (int j = 0; j < G1; ++j) {
            const double* rp = slot_ptr(G1 * g + j);
            x[j] = dbl2_t{k < Fc ? rp[k] : 0.0, k + 1 < Fc ? rp[k + 1] : 0.0};
        }
    };
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    auto stage_group = [&](const dbl2_t (&x)[G1], int g) {
#pragma unroll
        for (int j = 0; j < G1; ++j) {                                   // (slot t < 32: a row of the tile's 512 whatever nt is)
            const bf16x2_t h2 = {(__bf16)(float)x[j].x, (__bf16)(float)x[j].y};
            *reinterpret_cast<bf16x2_t*>(stage + (w + 16 * (G1 * g + j)) * CSEL_P1 + 4 * lane) = h2;
        }
    };
    // wave w multiplies a run of the product's row-major block list (the A operand is read again only where a block row starts)
    const int e0 = uni_i(w * nblk / 16), cntP = uni_i((w + 1) * nblk / 16 - e0);         // <= CSEL_MP
    f32x4_t acc[CSEL_MP], accD[2];
#pragma unroll
    for (int m = 0; m < CSEL_MP; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    accD[0] = accD[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int offA[CSEL_MP], offB[CSEL_MP], offD[2]; bool newRow[CSEL_MP];
#pragma unroll
    for (int m = 0; m < CSEL_MP; ++m) {
        const int e = min(e0 + m, e0 + cntP - 1), bx = e / nb2, by = e - bx * nb2;
        offA[m] = uni_i(16 * bx * CSEL_P1); offB[m] = uni_i((RB + 16 * by) * CSEL_P1);
        newRow[m] = uni_i((m == 0 || by == 0) ? 1 : 0) != 0;
    }
    offD[0] = uni_i(16 * min(w, nt - 1) * CSEL_P1); offD[1] = uni_i(16 * min(w + 16, nt - 1) * CSEL_P1);
    const int lanePart = (lane & 15) * CSEL_P1 + (lane >> 4) * 16;
    auto multiply = [&]() {
#pragma unroll
        for (int sub = 0; sub < KT / 32; ++sub) {
            const unsigned char* tb = stage + lanePart + 64 * sub;
            bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(tb + offA[0]);
#pragma unroll
            for (int m = 0; m < CSEL_MP; ++m)
                if (m < cntP) {
                    if (m > 0 && newRow[m]) a = *reinterpret_cast<const bf16x8_t*>(tb + offA[m]);
                    const bf16x8_t bq = *reinterpret_cast<const bf16x8_t*>(tb + offB[m]);
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq, acc[m], 0, 0, 0);
                }
#pragma unroll
            for (int m = 0; m < 2; ++m) {            // (staged rows: map 1's blocks, then map 2's)
                const bf16x8_t dg = *reinterpret_cast<const bf16x8_t*>(tb + offD[m]);
                accD[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dg, dg, accD[m], 0, 0, 0);
            }
        }
    };
    {
        dbl2_t xa[G1], xb[G1];
        if (NSF > 0) { load_group(xa, 0, 0); load_group(xb, 0, 1); }
        for (int st = 0; st < NSF; ++st) {
            for (int g = 0; g < NG8; g += 2) {
                // (the groups two ahead: the next tile's first two behind this tile's last — the last tile loads its own first two again)
                const int gn = g + 2 < NG8 ? g + 2 : 0, stn = g + 2 < NG8 ? st : min(st + 1, NSF - 1);
                stage_group(xa, g);
                load_group(xa, stn, gn);
                stage_group(xb, g + 1);
                load_group(xb, stn, gn + 1);
            }
            __syncthreads();
            multiply();
            __syncthreads();
        }
        if (NSF * KT < Fc) {                         // a ragged last tile: zeros behind the descriptor's end
            for (int g = 0; g < NG8; ++g) { load_group_ragged(xa, NSF, g); stage_group(xa, g); }
            __syncthreads();
            multiply();
            __syncthreads();
        }
    }
    // norms of the bf16 rows: element (r, r) of a diagonal block is register (lane & 3) of the lane with (lane & 15) >> 2 == lane >> 4
#pragma unroll
    for (int m = 0; m < 2; ++m)
        if (w + 16 * m < nt) {
            const int r4 = lane & 3;
            const float v = r4 == 0 ? accD[m][0] : r4 == 1 ? accD[m][1] : r4 == 2 ? accD[m][2] : accD[m][3];
            if (((lane & 15) >> 2) == (lane >> 4)) nrm[16 * (w + 16 * m) + (lane & 15)] = sqrt((double)v);
        }
    __syncthreads();
    CMARK(1);

    // ---- select -------------------------------------------------------------------------------------------
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int m = 0; m < CSEL_MP; ++m)
        if (m < cntP) {
            const int e = e0 + m, bx = e / nb2, by = e - bx * nb2;
            const int j = 16 * by + (lane & 15);
            const double nbv = nrm[RB + j];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = 16 * bx + 4 * (lane >> 4) + rr;
                const double na = nrm[i];
                const bool ok = i < n1 && j < n2;
                // (a row whose f32 norm is zero, tiny, huge or no number is left to the exact pass altogether: its guard for zero norms too)
                const double cv = (double)acc[m][rr] / (na * nbv);
                const bool cand = ok && (csel_unsafe(na) || csel_unsafe(nbv) || !(cv < thr));
                if (!LIVE && ok && !cand) cosPool[pd.cosOff + (int64_t)i * n2 + j] = cv;
                const unsigned long long bm = __ballot(cand);
                if (bm) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&hist[256], __popcll(bm));
                    base = __shfl(base, 0);
                    if (cand) {
                        const int slot = base + __popcll(bm & lt);
                        if (slot < CSEL_CAP) U[slot] = (uint32_t)i | ((uint32_t)j << 16);
                        atomicAdd(&hist[i], 1);
                    }
                }
            }
        }
    __syncthreads();
    const int nc = hist[256];
    if (nc > CSEL_CAP) { if (tid == 0) dense[b] = 1; return; }
    if (tid == 0) dense[b] = 0;
    if (nc == 0) { publish(0); return; }
    if (w == 0) {                                // cursors: exclusive prefix of the 256 row counts
        const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        int incl = c0 + c1 + c2 + c3;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        const int ex = incl - (c0 + c1 + c2 + c3);
        cur[4 * lane] = ex; cur[4 * lane + 1] = ex + c0; cur[4 * lane + 2] = ex + c0 + c1; cur[4 * lane + 3] = ex + c0 + c1 + c2;
    }
    __syncthreads();
    for (int q = tid; q < nc; q += 1024) { const uint32_t v = U[q]; S[atomicAdd(&cur[v & 0xffffu], 1)] = v; }
    __syncthreads();
    CMARK(2);

    // ---- pass 2 -------------------------------------------------------------------------------------------
    // The rows come again, chunk by chunk, as f64 (the same lanes, the same two register sets in flight).  The exact norms (the oracle's
    // stated order) are summed from the staged chunks: thread (r, h) takes chains 2 h and 2 h + 1 of row r.
    // (no branch inside the stream of loads, as in pass 1: every lane loads in each of the NQ rounds — behind the staged rows, or behind
    // its map's last object, the last real row again: a staged row that no candidate names)
    constexpr int NQ = CSEL_ROWS / 128;
    const int pp = lane & 7, laneRow = 8 * w + (lane >> 3);
    // (the launcher guarantees a feature pool of less than 4 GB: a lane's row is a 32-bit byte offset from the pool's start)
    uint32_t rofs[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int R = min(128 * q + laneRow, rowsTot - 1);
        const bool isA = R < RB;
        const int idx = min(isA ? R : R - RB, (isA ? n1 : n2) - 1);
        rofs[q] = (uint32_t)((((isA ? pd.off1 : pd.off2) + idx) * D.F + coff + 2 * pp) * 8);
    }
    const char* pool = reinterpret_cast<const char*>(feats);
    auto load16 = [&](dbl2_t (&x)[NQ], int k0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) { const d2u_t t = *reinterpret_cast<const d2u_t*>(pool + (rofs[q] + (uint32_t)(8 * k0))); x[q] = dbl2_t{t.v[0], t.v[1]}; }
    };
    auto load16_ragged = [&](dbl2_t (&x)[NQ], int k0) {
        const int k = k0 + 2 * pp;
#pragma unroll
        for (int q = 0; q < NQ; ++q) { const double* rb = reinterpret_cast<const double*>(pool + rofs[q]); x[q] = dbl2_t{k < Fc ? rb[k0] : 0.0, k + 1 < Fc ? rb[k0 + 1] : 0.0}; }
    };
    uint32_t my[CSEL_NPT]; double dot[CSEL_NPT];
    const int cnt2 = nc > tid ? (nc - tid + 1023) >> 10 : 0;
#pragma unroll
    for (int m = 0; m < CSEL_NPT; ++m) { my[m] = m < cnt2 ? S[m * 1024 + tid] : 0u; dot[m] = 0.0; }
    const int rN = tid >> 1, hN = tid & 1;
    double s0 = 0.0, s1 = 0.0;
    auto put16 = [&](const dbl2_t (&x)[NQ]) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            *reinterpret_cast<dbl2_t*>(stage + (128 * q + laneRow) * CSEL_P2 + 16 * pp) = x[q];
    };
    auto compute = [&](int s, auto fullChunk) {
        {   // (zeros behind a ragged descriptor's end: fma(0, 0, s) = s for a sum of squares)
            const dbl2_t* pr = reinterpret_cast<const dbl2_t*>(stage + rN * CSEL_P2 + 64 * hN);
            const dbl2_t e0_ = pr[0], e1_ = pr[1], e2_ = pr[2], e3_ = pr[3];
            s0 = fma(e0_.x, e0_.x, s0); s0 = fma(e0_.y, e0_.y, s0); s0 = fma(e1_.x, e1_.x, s0); s0 = fma(e1_.y, e1_.y, s0);
            s1 = fma(e2_.x, e2_.x, s1); s1 = fma(e2_.y, e2_.y, s1); s1 = fma(e3_.x, e3_.x, s1); s1 = fma(e3_.y, e3_.y, s1);
        }
        const int kleft = uni_i(Fc - 16 * s);    // elements of this chunk: >= 16 except the last of a ragged descriptor
#pragma unroll
        for (int m = 0; m < CSEL_NPT; ++m)
            if (m < cnt2) {
                const dbl2_t* pa = reinterpret_cast<const dbl2_t*>(stage + (my[m] & 0xffffu) * CSEL_P2);
                const dbl2_t* pb = reinterpret_cast<const dbl2_t*>(stage + (RB + (my[m] >> 16)) * CSEL_P2);
                double d = dot[m];
#pragma unroll
                for (int tp = 0; tp < 2; ++tp) {             // t = 2 tp, 2 tp + 1: the pairs (4 g + 2 tp, 4 g + 2 tp + 1), g = 0..3
                    dbl2_t av[4], bv[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) { av[g] = pa[2 * g + tp]; bv[g] = pb[2 * g + tp]; }
                    if (decltype(fullChunk)::value) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) d = fma(av[g].x, bv[g].x, d);
#pragma unroll
                        for (int g = 0; g < 4; ++g) d = fma(av[g].y, bv[g].y, d);
                    } else {
#pragma unroll
                        for (int g = 0; g < 4; ++g) if (4 * g + 2 * tp < kleft) d = fma(av[g].x, bv[g].x, d);
#pragma unroll
                        for (int g = 0; g < 4; ++g) if (4 * g + 2 * tp + 1 < kleft) d = fma(av[g].y, bv[g].y, d);
                    }
                }
                dot[m] = d;
            }
    };
    {
        const int NCF = Fc >> 4;                     // full chunks
        dbl2_t ya[NQ], yb[NQ];
        if (NCF > 0) { load16(ya, 0); load16(yb, 16 * min(1, NCF - 1)); }
        for (int s = 0; s < NCF; s += 2) {           // (two ahead; behind the last chunk that one again)
            put16(ya);
            __syncthreads();
            load16(ya, 16 * min(s + 2, NCF - 1));
            compute(s, std::true_type{});
            __syncthreads();
            if (s + 1 < NCF) {
                put16(yb);
                __syncthreads();
                load16(yb, 16 * min(s + 3, NCF - 1));
                compute(s + 1, std::true_type{});
                __syncthreads();
            }
        }
        if (NCF * 16 < Fc) {
            load16_ragged(ya, 16 * NCF);
            put16(ya);
            __syncthreads();
            compute(NCF, std::false_type{});
            __syncthreads();
        }
    }
    CMARK(3);
    // (LIVE: the live bits of the problem, 4 words per row of map 1, where pass 2's chunk was — every wave is behind its last barrier)
    unsigned long long* liveBits = reinterpret_cast<unsigned long long*>(stage);
    static_assert(CSEL_MAXN * (CSEL_MAXN / 64) <= 1024 && CSEL_MAXN * (CSEL_MAXN / 64) * 8 <= CSEL_ROWS * CSEL_P2, "one word per thread, in pass 2's chunk");
    if (LIVE) liveBits[tid] = 0ull;
    {
        const double p = s0 + s1, q = __shfl_xor(p, 1);
        if (hN == 0) nrm[rN] = sqrt(p + q);      // (s0 + s1) + (s2 + s3)
    }
    __syncthreads();
    double sc[CSEL_NPT];
    bool live[CSEL_NPT];
#pragma unroll
    for (int m = 0; m < CSEL_NPT; ++m) {
        live[m] = false; sc[m] = 0.0;
        if (m < cnt2) {
            const int i = (int)(my[m] & 0xffffu), j = (int)(my[m] >> 16);
            const double na = nrm[i], nbv = nrm[RB + j];
            const double cosv = (na > 0.0 && nbv > 0.0) ? dot[m] / (na * nbv) : 0.0;
            if (!LIVE) cosPool[pd.cosOff + (int64_t)i * n2 + j] = cosv;
            // k_live<0>'s gate and full score on the exact cosine (a non-candidate fails the gate: see above)
            else if ((cosv - D.p.cosine_min) / (D.p.cosine_max - D.p.cosine_min) > 0.0) {
                const int pdm = D.p.point_dim;
                const double* fi = feats + (pd.off1 + i) * D.F + pdm; const double* fj = feats + (pd.off2 + j) * D.F + pdm;
                sc[m] = single_score(D, [&](int f) { return fi[f]; }, [&](int f) { return fj[f]; }, cosv);
                live[m] = sc[m] > 0.0;
                if (live[m]) atomicOr(&liveBits[4 * i + (j >> 6)], 1ull << (j & 63));
            }
        }
    }
    if (!LIVE) { CMARK(4); }
    else {
        // ordered compaction: the live association (i, j) goes to position (live in rows < i) + (live in row i at columns < j) — ascending
        // association index i n2 + j, whatever order the candidates arrived in
        __syncthreads();
        if (w == 0) {                            // row bases: exclusive prefix of the 256 row counts; cur[256]: the problem's total
            int c4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long* rw = liveBits + 4 * (4 * lane + k);
                c4[k] = __popcll(rw[0]) + __popcll(rw[1]) + __popcll(rw[2]) + __popcll(rw[3]);
            }
            int incl = c4[0] + c4[1] + c4[2] + c4[3];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
            const int ex = incl - (c4[0] + c4[1] + c4[2] + c4[3]);
            cur[4 * lane] = ex; cur[4 * lane + 1] = ex + c4[0]; cur[4 * lane + 2] = ex + c4[0] + c4[1]; cur[4 * lane + 3] = ex + c4[0] + c4[1] + c4[2];
            if (lane == 63) cur[256] = incl;
        }
        __syncthreads();
        const int64_t lo = pd.liveOff;
        const bool has_z = D.p.point_dim == 3;
#pragma unroll
        for (int m = 0; m < CSEL_NPT; ++m)
            if (live[m]) {
                const int i = (int)(my[m] & 0xffffu), j = (int)(my[m] >> 16), wj = j >> 6;
                const unsigned long long* rw = liveBits + 4 * i;
                int pos = cur[i] + __popcll(rw[wj] & ((1ull << (j & 63)) - 1ull));
                for (int k = 0; k < wj; ++k) pos += __popcll(rw[k]);
                const double s = sc[m];
                lv.lp[lo + pos] = i * n2 + j; lv.li[lo + pos] = i; lv.lj[lo + pos] = j; lv.ls[lo + pos] = s;
                lv.ld[lo + pos] = D.diag_one ? 1.0 : s;
                lv.lza[lo + pos] = has_z ? feats[(pd.off1 + i) * D.F + 2] : 0.0;
                lv.lzb[lo + pos] = has_z ? feats[(pd.off2 + j) * D.F + 2] : 0.0;
            }
        publish(cur[256]);
        CMARK(4);
    }
#ifdef ROMAN_CSEL_TIMING
    if (tid == 0 && (b & 63) == 0) printf("[%s] b=%d candidates=%d cycles: pass1 %llu select %llu pass2 %llu tail %llu\n", LIVE ? "k_cos_live" : "k_cos_sel", b, nc,
                                          tc_[1] - tc_[0], tc_[2] - tc_[1], tc_[3] - tc_[2], tc_[4] - tc_[3]);
#endif
#undef CMARK
}

__global__ void __launch_bounds__(1024) k_cos_sel(DevParams D, int B, const ProbDesc* __restrict__ probs, const double* __restrict__ feats,
                                                  double* __restrict__ cosPool, int32_t* __restrict__ dense /* [B] out: 1 = left to the dense kernel */,
                                                  double thr /* cosine_min - delta; +inf: no candidates (the approximate matrix, tests) */)
{
    cos_sel_body<false>(D, B, probs, feats, cosPool, dense, thr, CselLive{});
}

// ---------------------------------------------------------------------------------------------
// k_cos_live: the cosine stage AND k_live<0> + k_live<1> of a batch of all-to-all problems (assocOff < 0) whose single scores are gated
// (the conditions of k_cos_sel, and not keep_all) in one workgroup per problem: k_cos_sel's passes (the same screen and bound, the
// same candidates, cosines bit-identical to k_cos_deal's), then, for every candidate, k_live<0>'s gate on its exact cosine and
// single_score() with the same operands, and the problem's live pools in ascending association index with L / kind / nnzUpper as
// k_live<1> writes them.  Non-candidates fail the gate (their exact cosine is below cosine_min).  No cosine matrix is written: the
// 8 bytes per pair of the batch that k_live<0> read back only to gate.  A problem flagged in dense[] (more than CSEL_CAP candidates,
// maps beyond the block budget) is left whole to k_cos_deal + k_live, which the launcher runs behind this kernel for those only.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_cos_live(DevParams D, int B, const ProbDesc* __restrict__ probs, const double* __restrict__ feats,
                                                   int32_t* __restrict__ dense /* [B] out: 1 = left to the dense kernels */, double thr /* cosine_min - delta */,
                                                   ProbState* __restrict__ st, int32_t* __restrict__ lp, int32_t* __restrict__ li, int32_t* __restrict__ lj,
                                                   double* __restrict__ ls, double* __restrict__ ld, double* __restrict__ lza, double* __restrict__ lzb)
{
    cos_sel_body<true>(D, B, probs, feats, nullptr, dense, thr, CselLive{st, lp, li, lj, ls, ld, lza, lzb});
}

// ---------------------------------------------------------------------------------------------
// k_tables: TA[i][i'] (n1 x n1) and TB[j][j'] (n2 x n2).  Entry = horizontal distance (gravity)
// or full distance (otherwise) between two objects of the same map; NaN when the two objects
// coincide (distinctness) or are closer than mindist — every comparison against NaN is false, so
// one table lookup implements the distinctness skip, the mindist gate and the distance itself.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_tables(DevParams D, const ProbDesc* __restrict__ probs,
                                                 const double* __restrict__ feats,
                                                 double* __restrict__ tabPool, int RB /* rows per band */,
                                                 uint16_t* __restrict__ qtabPool /* the same entries as 15-bit bins of width epsilon / 32 (k_count's prefilter), or NULL */)
{
    // grid: (row bands of RB rows over max(n1,n2), 2 maps, B).  The map's points are staged in LDS once per
    // block (3 doubles per object: n gathers from rows 8 F bytes apart — the band is as tall as the batch allows, one band
    // per map when there are enough problems to fill the device); a wave writes table rows with lanes along the row (coalesced).
    extern __shared__ __attribute__((aligned(16))) double s_xyz[];
    const ProbDesc pd = probs[blockIdx.z];
    const int which = blockIdx.y;
    const int n = which == 0 ? pd.n1 : pd.n2;
    const int r0 = blockIdx.x * RB;
    if (r0 >= n) return;
    const int64_t base = which == 0 ? pd.off1 : pd.off2;
    const int pdim = D.p.point_dim;
    for (int t = threadIdx.x; t < n * 3; t += blockDim.x) {
        const int o = t / 3, c = t - o * 3;
        s_xyz[t] = (c < pdim) ? feats[(base + o) * D.F + c] : 0.0;
    }
    __syncthreads();
    double* tab = tabPool + pd.tabOff + (which == 0 ? 0 : (int64_t)pd.n1 * pd.n1);
    const int nq = (n + 3) & ~3;                                  // row stride of the bins (a row is whole 8-byte words)
    uint16_t* qtab = qtabPool ? qtabPool + 4 * (int64_t)pd.qtabOff4 + (which == 0 ? 0 : (int64_t)pd.n1 * ((pd.n1 + 3) & ~3)) : nullptr;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int rr = w; rr < RB; rr += nw) {
        const int a = r0 + rr;
        if (a >= n) break;
        const double ax = s_xyz[3 * a], ay = s_xyz[3 * a + 1], az = s_xyz[3 * a + 2];
        for (int b = lane; b < n; b += WAVE) {
            const double dx = ax - s_xyz[3 * b], dy = ay - s_xyz[3 * b + 1], dz = az - s_xyz[3 * b + 2];
            const double h2 = dx * dx + dy * dy;
            const double l2 = h2 + dz * dz;
            const bool bad = (a == b) || (D.p.mindist > 0.0 && l2 < D.x_mindist);
            const double v = (D.gmode == 1 || D.gmode == 2) ? sqrt(h2) : sqrt(l2);     // z-gate mode compares full lengths
            tab[(int64_t)a * n + b] = bad ? d_nan() : v;
            // NaN entries and everything beyond the bins' range share the last bin (fmin returns the number)
            if (qtab) qtab[(int64_t)a * nq + b] = (uint16_t)(uint32_t)__builtin_fmin((bad ? d_nan() : v) * D.pre_invw, 32767.0);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_live<PHASE>: single score of every association and ordered (ascending association index)
// compaction of the live ones, in two launches over chunks of LIVE_CHUNK associations (grid:
// chunks x problems, so a single problem is spread over many CUs as well):
//   PHASE 0  every wave owns a contiguous quarter of the chunk (a segment) and leaves the segment's live associations
//            (index, score; in order) at the head of the segment's slice of a scratch pool, their number in segCnt
//   PHASE 1  segment base = sum of the counts in front of it (fixed order), copy into the live pools; the
//            workgroup of chunk 0 also publishes L.
// ---------------------------------------------------------------------------------------------
constexpr int LIVE_CHUNK = 4096;

template <int PHASE>
__global__ void __launch_bounds__(256) k_live(DevParams D, const ProbDesc* __restrict__ probs,
                                              ProbState* __restrict__ st,
                                              const double* __restrict__ feats,
                                              const int32_t* __restrict__ assoc,
                                              const double* __restrict__ cosPool,
                                              double* __restrict__ qS, int32_t* __restrict__ qP /* the segments' live associations: score, index */,
                                              int32_t* __restrict__ segCnt, int maxChunks,
                                              int32_t* __restrict__ lp, int32_t* __restrict__ li,
                                              int32_t* __restrict__ lj, double* __restrict__ ls, double* __restrict__ ld,
                                              double* __restrict__ lza, double* __restrict__ lzb,
                                              const int32_t* __restrict__ only /* NULL, or [B]: problems with a 0 are skipped (k_cos_live completed them) */)
{
    __shared__ int cbase[2];
    __shared__ uint16_t survQ[PHASE == 0 ? 4 : 1][PHASE == 0 ? LIVE_CHUNK / 4 : 1];     // phase 0: per wave, the associations behind the cosine gate
    const int b = blockIdx.y, c = blockIdx.x;
    if (only && !only[b]) return;
    const ProbDesc pd = probs[b];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int nA = pd.nA;
    const int nChunks = (nA + LIVE_CHUNK - 1) / LIVE_CHUNK;
    if (c >= nChunks && !(PHASE == 1 && c == 0)) return;
    constexpr int SEG = LIVE_CHUNK / 4;                          // associations per wave (blockDim.x == 256)
    constexpr int NIT = SEG / WAVE;
    const int p_beg = min(nA, c * LIVE_CHUNK + w * SEG), p_end = min(nA, p_beg + SEG);
    const int Fc = D.p.cos_feature_dim;
    const int64_t lo = pd.liveOff;
    int32_t* sc = segCnt + (int64_t)b * maxChunks * 4;           // live associations per wave segment, in association order
    const unsigned long long lt = (1ull << lane) - 1ull;

    if (PHASE == 0) {
        // The wave leaves its segment's LIVE associations — index and score, in order — at the head of the segment's slice
        // of (qP, qS), and their number in segCnt: nothing is written for the ~95 % that fail (a score array over all
        // associations, written here and read back by phase 1, was 2 x 84 MB per batch of 256 at config 3 — these two
        // kernels' whole time).  With a cosine term the cheap part of the score is a gate: the wave first sweeps its
        // segment with the gate alone (all cosine loads in flight together), queues the survivors in LDS, and then
        // evaluates the full score — ratios, roots, fusion: ~250 f64 instructions — for the survivors only, 64 at a time.
        // single_score() returns 0 for an association that fails the gate whatever its ratios are, so nothing changes.
        const int pdm = D.p.point_dim;
        auto full_score = [&](int p) {
            int i, j;
            decode_assoc(pd, assoc, p, i, j);
            const double cosv = (Fc > 0) ? cosPool[pd.cosOff + (int64_t)i * pd.n2 + j] : 0.0;
            const double* fi = feats + (pd.off1 + i) * D.F + pdm; const double* fj = feats + (pd.off2 + j) * D.F + pdm;
            return single_score(D, [&](int f) { return fi[f]; }, [&](int f) { return fj[f]; }, cosv);
        };
        int nlive = 0;
        auto emit = [&](bool valid, int p, double s) {          // ordered append of the lanes with a live association
            const bool live = valid && (s > 0.0 || D.keep_all || D.plain_all);
            const unsigned long long m = __ballot(live);
            if (live) { const int k = p_beg + nlive + __popcll(m & lt); qP[lo + k] = p; qS[lo + k] = s; }
            nlive += __popcll(m);
        };
        if (D.single && Fc > 0 && !D.keep_all && !D.plain_all) {
            uint16_t* q = survQ[w];
            const double cden = D.p.cosine_max - D.p.cosine_min;
            int ns = 0;
            double cv[NIT];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int p = p_beg + it * WAVE + lane;
                cv[it] = 0.0;
                if (p < p_end) {
                    int i, j;
                    decode_assoc(pd, assoc, p, i, j);
                    cv[it] = cosPool[pd.cosOff + (int64_t)i * pd.n2 + j];
                }
            }
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int p = p_beg + it * WAVE + lane;
                const bool pass = p < p_end && (D.pruned ? !(cv[it] < D.p.cosine_min) : ((cv[it] - D.p.cosine_min) / cden > 0.0));
                const unsigned long long m = __ballot(pass);
                if (pass) q[ns + __popcll(m & lt)] = (uint16_t)(p - p_beg);
                ns += __popcll(m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int k0 = 0; k0 < ns; k0 += WAVE) {
                const int k = k0 + lane;
                const int p = p_beg + (int)q[min(k, max(ns - 1, 0))];
                emit(k < ns, p, k < ns ? full_score(p) : 0.0);
            }
        } else {
            for (int p0 = p_beg; p0 < p_end; p0 += WAVE) {
                const int p = p0 + lane;
                emit(p < p_end, p, (p < p_end && D.single) ? full_score(p) : 1.0);
            }
        }
        if (lane == 0) sc[c * 4 + w] = nlive;
        return;
    }

    // PHASE 1
    if (w == 0) {                                               // live associations in front of this chunk, and the problem total
        int front = 0, total = 0;
        for (int k0 = 0; k0 < nChunks * 4; k0 += WAVE) {
            const int k = k0 + lane;
            const int v = k < nChunks * 4 ? sc[k] : 0;
            int f = k < c * 4 ? v : 0, t = v;
            for (int off = 32; off > 0; off >>= 1) { f += __shfl_xor(f, off); t += __shfl_xor(t, off); }
            front += f; total += t;
        }
        if (lane == 0) { cbase[0] = front; cbase[1] = total; }
    }
    __syncthreads();
    // ROMAN_INV_EUCLIDEAN_PRUNED with NO survivor: the reference hands clipperpy an empty list, i.e. the all-to-all one
    const bool all_live = D.pruned && cbase[1] == 0 && nA > 0;
    const int Ltot = all_live ? nA : cbase[1];
    if (c == 0 && tid == 0) {
        st[b].L = Ltot; st[b].nnzUpper = 0ull;
        st[b].kind = live_kind(D, Ltot);
    }
    if (c >= nChunks) return;
    int base = cbase[0];
    for (int k = 0; k < w; ++k) base += sc[c * 4 + k];
    const int n = all_live ? p_end - p_beg : sc[c * 4 + w];
    if (all_live) base = p_beg;                                 // live index == association index
    const bool has_z = D.p.point_dim == 3;
    for (int k0 = 0; k0 < n; k0 += WAVE) {
        const int k = k0 + lane;
        if (k < n) {
            const int p = all_live ? p_beg + k : qP[lo + p_beg + k];
            const double s = all_live ? 1.0 : qS[lo + p_beg + k];
            int i, j;
            decode_assoc(pd, assoc, p, i, j);
            const int pos = base + k;
            lp[lo + pos] = p; li[lo + pos] = i; lj[lo + pos] = j; ls[lo + pos] = s;
            ld[lo + pos] = D.diag_one ? 1.0 : s;               // M_pp: the single score, or the identity (ROMAN_SINGLE_OFFDIAG)
            lza[lo + pos] = has_z ? feats[(pd.off1 + i) * D.F + 2] : 0.0;
            lzb[lo + pos] = has_z ? feats[(pd.off2 + j) * D.F + 2] : 0.0;
        }
    }
}

// k_rowbase: prefix of the live counts over the problems of the batch; also the batch maxima, the offsets of
// the per-problem candidate bit matrices (L rows of ceil(L/64) words) and the work-item prefix
// (a work item = a block of up to RPB consecutive live rows of one problem).  The bit-matrix pools were sized
// before L was known: a problem whose matrix would end beyond `capMaskWords` becomes kind 2 (skipped).
// Block-wide exclusive prefix sum (blockDim.x a multiple of 64, <= 1024): every thread gets the sum of the values of the
// threads in front of it, `total` the sum over the block.  sh: 17 elements of scratch; two barriers.
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* sh, T& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    T inc = v;
    for (int off = 1; off < WAVE; off <<= 1) { const T t = __shfl_up(inc, off); if (lane >= off) inc += t; }
    __syncthreads();                                             // (sh may still be read from the previous call)
    if (lane == WAVE - 1) sh[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int k = 0; k < nw; ++k) { const T x = sh[k]; if (k < w) base += x; tot += x; }
    total = tot;
    return base + inc - v;
}

__global__ void __launch_bounds__(1024) k_rowbase(int B, int RPB, long long capMaskWords, ProbState* __restrict__ st, BatchTotals* __restrict__ tot,
                                                  int smallOnly /* the general kernels are not launched: what k_small left behind is skipped */,
                                                  const int32_t* __restrict__ cosDense /* NULL, or k_cos_sel's flags of the batch */)
{
    // one workgroup; a thread takes PER consecutive problems (a serial sweep of one wave over 4096 problems was 93 us —
    // 64 dependent round trips to memory — of the 1.4 ms the whole batch takes at the reference's demo scale)
    __shared__ long long shl[17];
    __shared__ int shi[17];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int PER = (B + nt - 1) / nt;
    const int b0 = tid * PER, b1 = min(B, b0 + PER);
    // the thread's problems are read ONCE (up to PC of them are kept in registers: the three sweeps below would otherwise be
    // three dependent round trips to memory each)
    constexpr int PC = 8;
    int cL[PC], cK[PC];
#pragma unroll
    for (int j = 0; j < PC; ++j) { const int b = b0 + j; const bool in = j < PER && b < b1; cL[j] = in ? st[b].L : 0; cK[j] = in ? st[b].kind : 2; }
    auto getL = [&](int b) { const int j = b - b0; int v = 0; if (j < PC) {
#pragma unroll
        for (int t = 0; t < PC; ++t) if (t == j) v = cL[t]; } else v = st[b].L; return v; };
    auto getK = [&](int b) { const int j = b - b0; int v = 2; if (j < PC) {
#pragma unroll
        for (int t = 0; t < PC; ++t) if (t == j) v = cK[t]; } else v = st[b].kind; return v; };
    long long sM = 0, sN = 0; int sR = 0;
    for (int b = b0; b < b1; ++b) {
        const int L = getL(b);
        const long long mwAll = (long long)L * ((L + 63) >> 6);
        sN += mwAll; sR += L;
        if (getK(b) < 2) sM += mwAll;                            // kind 2: already skipped (k_live: no fallback kernels in this launch); kind 3: finished by k_small
    }
    long long totM, totN; int totR, totI;
    const long long baseM = block_excl_scan(sM, shl, totM);
    (void)block_excl_scan(sN, shl, totN);
    const int baseR = block_excl_scan(sR, shi, totR);
    // the prefix is monotone: once a problem does not fit, none behind it does
    int sI = 0;
    {
        long long accM = baseM;
        for (int b = b0; b < b1; ++b) {
            const int L = getL(b);
            const bool skip = getK(b) >= 2;
            const long long mw = skip ? 0 : (long long)L * ((L + 63) >> 6);
            accM += mw;
            if (!skip && accM <= capMaskWords) sI += (L + RPB - 1) / RPB;
        }
    }
    const int baseI = block_excl_scan(sI, shi, totI);
    int mx = 0, mxs = 0, nover = 0, mns = 0x7fffffff, ngen = 0, ndense = 0;
    {
        long long accM = baseM; int accR = baseR, accI = baseI;
        for (int b = b0; b < b1; ++b) {
            if (cosDense) ndense += cosDense[b] != 0;
            const int L = getL(b);
            const int kind = getK(b);
            const bool skip = kind >= 2;
            const long long mw = skip ? 0 : (long long)L * ((L + 63) >> 6);
            const bool fits = !skip && !smallOnly && accM + mw <= capMaskWords;
            const int it = fits ? (L + RPB - 1) / RPB : 0;
            st[b].rowBase = accR; st[b].itemBase = accI; st[b].maskOff = fits ? accM : 0;
            if (kind < 2) ++ngen;                                // (also when it is skipped here: the history must learn that the general kernels are needed)
            if (kind == 3) mns = min(mns, L);                    // finished by k_small: still a small problem the history should know of
            else if (!fits) {                                    // (also a problem k_live already skipped: no fallback kernels in this launch)
                st[b].kind = 2; ++nover;
                // skipped only because the general kernels were left out (small_only): the history learns its size NOW, so that the
                // second attempt sizes the solver launch for it instead of spending one more attempt on that
                if (smallOnly && kind == 0) { mxs = max(mxs, L); mns = min(mns, L); }
            }
            else if (kind == 0) { mxs = max(mxs, L); mns = min(mns, L); }
            mx = max(mx, L);
            accM += mw; accR += L; accI += it;
        }
    }
    // batch maxima / counts: wave reduction, then one atomic per wave on LDS words
    __shared__ int red[6];
    if (tid == 0) { red[0] = 0; red[1] = 0; red[2] = 0; red[3] = 0x7fffffff; red[4] = 0; red[5] = 0; }
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) { mx = max(mx, __shfl_xor(mx, off)); mxs = max(mxs, __shfl_xor(mxs, off)); nover += __shfl_xor(nover, off); mns = min(mns, __shfl_xor(mns, off)); ngen += __shfl_xor(ngen, off); ndense += __shfl_xor(ndense, off); }
    if ((tid & 63) == 0) { atomicMax(&red[0], mx); atomicMax(&red[1], mxs); atomicAdd(&red[2], nover); atomicMin(&red[3], mns); atomicAdd(&red[4], ngen); atomicAdd(&red[5], ndense); }
    __syncthreads();
    if (tid == 0) {
        tot->cosScreened = cosDense ? B : 0; tot->cosDense = red[5];
        tot->R = totR; tot->maxL = red[0]; tot->nnzTotal = 0; tot->maskWords = totM < capMaskWords ? totM : capMaskWords; tot->items = totI; tot->sliceGroups = 0;
        tot->needMaskWords = totN; tot->needNnz = 0; tot->overflow = red[2]; tot->maxStreamL = red[1]; tot->minStreamL = red[3]; tot->nGeneral = red[4]; tot->listTop = 0ull;
    }
}

// k_items: the work-item list of the pair-test and fill kernels.
__global__ void __launch_bounds__(256) k_items(int RPB, const ProbState* __restrict__ st, ItemDesc* __restrict__ items)
{
    const int b = blockIdx.x;
    const int L = st[b].L, ib = st[b].itemBase;
    const int n = (st[b].kind >= 2) ? 0 : (L + RPB - 1) / RPB;
    for (int t = threadIdx.x; t < n; t += blockDim.x) { ItemDesc d; d.b = b; d.row0 = t * RPB; items[ib + t] = d; }
}

// ---------------------------------------------------------------------------------------------
// k_count: the O(L^2) pair tests of the affinity build, done ONCE.  A workgroup takes a work item
// (RPB consecutive live rows of one problem) and stages the problem's COLUMN data (map-1/map-2
// object and the two z coordinates of every live association) in LDS once; each wave then owns a
// row k=(i,j) at a time: it stages the two table rows TA[i][:] and TB[j][:] in its private LDS
// slice and sweeps the live columns 64 at a time.  A test costs three coalesced LDS reads, two LDS
// gathers and ~12 f64 VALU ops, all exactly rounded (+,-,*,compare).  Output per row: the candidate
// bit mask (one ballot word per 64 columns), the running candidate count in front of every word
// (k_fill turns it into the entry index without another scan) and the row total.
// A live set that does not fit the LDS column tile is swept tile by tile.
// ---------------------------------------------------------------------------------------------
// exclusive prefix sum over the 64 lanes of a wave
// (DPP: six VALU instructions — row_shr:1,2,4,8 inside the rows of 16 lanes, row_bcast:15 / :31 across them; lanes without a
// source add the `old` operand, 0.  The __shfl_up form compiles to six DEPENDENT ds_bpermute round trips through the LDS
// crossbar, ~500 cycles of latency per scan: k_upper spends one scan per matrix row.)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, int lane) { (void)lane; return wave_incl_scan(v) - v; }

// lane `sel` of (hi:lo) <- the wave-uniform 64-bit value m (two v_writelane_b32: uniform value, uniform lane select).  The
// instruction's constant bus takes one SGPR: the lane select travels in m0.  This compiler exposes no writelane builtin, and
// m0 is a reserved register that an asm statement may not list as clobbered: the statement saves and restores it itself.
__device__ __forceinline__ void writelane2(uint32_t& lo, uint32_t& hi, unsigned long long m, uint32_t sel)
{
    const uint32_t ml_ = (uint32_t)m, mh_ = (uint32_t)(m >> 32);
    uint32_t keep_;
    asm("s_mov_b32 %2, m0\n\ts_mov_b32 m0, %4\n\tv_writelane_b32 %0, %3, m0\n\tv_writelane_b32 %1, %5, m0\n\ts_mov_b32 m0, %2"
        : "+v"(lo), "+v"(hi), "=&s"(keep_) : "s"(ml_), "s"(sel), "s"(mh_));
}

// GM: 0 no gravity prior, 1 ROMAN_GRAV_COMBINED, 2 ROMAN_GRAV_SEPARATE, 3 ROMAN_GRAV_ZGATE (tables then hold full lengths)
template <int GM>
__device__ __forceinline__ bool pair_gate(const DevParams& D, double a, double bb, double dz)
{
    if (GM == 1) {
        const double ch = fabs(a - bb);
        double hm;                              // max(a,bb) in ONE instruction (fmax() would first
        asm("v_max_f64 %0, %1, %2" : "=v"(hm) : "v"(a), "v"(bb));   // canonicalise both); NaN operands: x is NaN through ch anyway
        const double cv = __builtin_fmax(dz - D.sin_unc * hm, 0.0);
        const double xx = ch * ch + cv * cv;
        return xx < D.x_eps;                    // <=> sqrt(x) < epsilon ; NaN -> false
    } else if (GM == 2) {
        const double ch = fabs(a - bb);
        double hm;
        asm("v_max_f64 %0, %1, %2" : "=v"(hm) : "v"(a), "v"(bb));
        const double cv = __builtin_fmax(dz - D.sin_unc * hm, 0.0);
        return (ch < D.p.epsilon) & (cv < D.p.epsilon);             // a NaN table entry fails through ch
    } else if (GM == 3) {
        const double c = fabs(a - bb);
        double lm;
        asm("v_max_f64 %0, %1, %2" : "=v"(lm) : "v"(a), "v"(bb));
        return (c < D.p.epsilon) & (dz < D.p.epsilon + D.sin_unc * lm);
    } else {
        return fabs(a - bb) < D.p.epsilon;
    }
}

// Fast sweep: columns in LDS as the packed pair {i_q, n1+1+j_q} of indices into a table slice (+ the two z
// coordinates), padded to a multiple of 256 columns with a sentinel whose table entry is NaN (fails every
// test), so the inner loop has no bounds logic at all.  A wave sweeps NR ADJACENT rows at once (NR = 2 when
// the table slices fit): the column data is read once for both, the two rows' instruction streams are
// independent (the kernel is bound by LDS/VALU/scalar latency, not by any one pipe), and the loop overhead
// is shared.  Per 64 columns and row: 2 LDS gathers, 12 f64 VALU ops, 2 address adds, 2 v_writelane.
template <int GM, int NR, bool TILED>
__device__ __forceinline__ void count_rows_lds(const DevParams& D, const ProbDesc& pd, int L, int row0, int nrows,
                                               int w, int wpb, int lane,
                                               const uint32_t* cIJ /* i_q | (n1 + 1 + j_q) << 16: table-slice indices */, const double2* cZZ,
                                               const double* __restrict__ TA, const double* __restrict__ TB,
                                               double* tA /* NR slices of ldsPerRow doubles */, int ldsPerRow,
                                               unsigned long long* __restrict__ mbase,
                                               int c0_ /* first column of the LDS tile */, int clen /* its columns (multiple of 256) */,
                                               const int32_t* __restrict__ gI, const int32_t* __restrict__ gJ,
                                               const double* __restrict__ gZa, const double* __restrict__ gZb /* the rows' own data when the tile does not hold them (c0 > 0 or clen < Lpad) */)
{
    const int W = (L + 63) >> 6;
    // TILED == false: the tile holds the whole live set (c0 = 0 folds away: the sweep is the one-tile code of rounds 1-3)
    constexpr bool tiled = TILED;
    const int c0 = TILED ? c0_ : 0;
    const int cend = TILED ? c0 + clen : 0x7fffffff;
    const char* tbytes = reinterpret_cast<const char*>(tA);
    const int sliceBytes = ldsPerRow * 8;
    constexpr int U = 2;                                        // column chunks per step (with 2 rows per wave: 2 beats 1 and 4)
    const int Lpad = (L + U * WAVE - 1) & ~(U * WAVE - 1);
    // Rows are columns too: their objects and z come from the LDS column tile.  The table rows of the NEXT
    // rows are fetched into registers while the current ones are swept (maps of up to 256 objects; larger ones
    // load directly), so no global-memory latency sits between two sweeps.
    constexpr int TR = 4;
    const bool pre = pd.n1 <= TR * WAVE && pd.n2 <= TR * WAVE;
    double ra[NR][TR], rb[NR][TR];
    auto fetch_tab = [&](int r_) {
#pragma unroll
        for (int x = 0; x < NR; ++x) {
            const int k_ = row0 + min(r_ + x, nrows - 1);
            const int i_ = tiled ? gI[k_] : (int)(cIJ[k_] & 0xffffu), j_ = tiled ? gJ[k_] : (int)(cIJ[k_] >> 16) - (pd.n1 + 1);
            const double* gA_ = TA + (int64_t)i_ * pd.n1;
            const double* gB_ = TB + (int64_t)j_ * pd.n2;
#pragma unroll
            for (int m_ = 0; m_ < TR; ++m_) {
                ra[x][m_] = (lane + m_ * WAVE < pd.n1) ? gA_[lane + m_ * WAVE] : 0.0;
                rb[x][m_] = (lane + m_ * WAVE < pd.n2) ? gB_[lane + m_ * WAVE] : 0.0;
            }
        }
    };
    if (pre && NR * w < nrows) fetch_tab(__builtin_amdgcn_readfirstlane(NR * w));
    for (int r = NR * w; r < nrows; r += NR * wpb) {
        int k[NR]; double zi[NR], zj[NR];
#pragma unroll
        for (int x = 0; x < NR; ++x) {
            k[x] = __builtin_amdgcn_readfirstlane(row0 + min(r + x, nrows - 1));   // wave-uniform: loop bounds and lane selects in SGPRs
            zi[x] = GM ? (tiled ? gZa[k[x]] : cZZ[k[x]].x) : 0.0; zj[x] = GM ? (tiled ? gZb[k[x]] : cZZ[k[x]].y) : 0.0;
        }
        // stage the table rows (wave-private slices; LDS ops of one wave execute in order)
#pragma unroll
        for (int x = 0; x < NR; ++x) {
            double* sA = tA + x * ldsPerRow; double* sB = sA + pd.n1 + 1;
            if (pre) {
#pragma unroll
                for (int m_ = 0; m_ < TR; ++m_) {
                    if (lane + m_ * WAVE < pd.n1) sA[lane + m_ * WAVE] = ra[x][m_];
                    if (lane + m_ * WAVE < pd.n2) sB[lane + m_ * WAVE] = rb[x][m_];
                }
            } else {
                const int i = tiled ? gI[k[x]] : (int)(cIJ[k[x]] & 0xffffu), j = tiled ? gJ[k[x]] : (int)(cIJ[k[x]] >> 16) - (pd.n1 + 1);
                const double* gA = TA + (int64_t)i * pd.n1;
                const double* gB = TB + (int64_t)j * pd.n2;
                for (int t = lane; t < pd.n1; t += WAVE) sA[t] = gA[t];
                for (int t = lane; t < pd.n2; t += WAVE) sB[t] = gB[t];
            }
            if (lane == 0) sA[pd.n1] = d_nan();                 // sentinel entry of the padding columns
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (pre && r + NR * wpb < nrows) fetch_tab(__builtin_amdgcn_readfirstlane(r + NR * wpb));

        // The pair test is symmetric: row k computes only the 64-column words c >= R = k/64 (the diagonal word
        // completely, both of its triangles); the words c < R are the bit transposes of blocks computed by other
        // rows and are written by k_mirror.  Prefix counts and row totals are taken afterwards by k_rowprefix.
        // The NR rows of a wave are adjacent and start at a multiple of NR: they lie in the same 64-row block.
        const int R = k[0] >> 6;
        uint32_t mlo[NR], mhi[NR];                              // lane l: word (block*64 + l) of the current 64-word block
#pragma unroll
        for (int x = 0; x < NR; ++x) { mlo[x] = 0u; mhi[x] = 0u; }
        const int qEnd = TILED ? min(Lpad, cend) : Lpad;        // (a live set larger than the LDS tile is swept tile by tile: k_count)
        for (int q0 = max((R << 6) & ~(U * WAVE - 1), c0); q0 < qEnd; q0 += U * WAVE) {
            int2 ij[U]; double2 zz[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const uint32_t pk = cIJ[q0 - c0 + t * WAVE + lane];
                ij[t] = make_int2((int)((pk & 0xffffu) << 3), (int)((pk >> 16) << 3));     // byte offsets into a table slice
                if (GM) zz[t] = cZZ[q0 - c0 + t * WAVE + lane];
            }
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const int widx = TILED ? uni_i((q0 >> 6) + t) : (q0 >> 6) + t;   // words >= W are all-zero (sentinel columns); (out-of-line tiled path: arguments arrive in vector registers)
#pragma unroll
                for (int x = 0; x < NR; ++x) {
                    const double a = *reinterpret_cast<const double*>(tbytes + x * sliceBytes + ij[t].x);
                    const double bb = *reinterpret_cast<const double*>(tbytes + x * sliceBytes + ij[t].y);
                    const double dz = GM ? fabs((zi[x] - zz[t].x) - (zj[x] - zz[t].y)) : 0.0;
                    const bool is = pair_gate<GM>(D, a, bb, dz);
                    const unsigned long long m = __ballot(is);
                    // lane (widx & 63) of (mhi:mlo) <- m
                    writelane2(mlo[x], mhi[x], m, (uint32_t)(widx & 63));
                }
            }
            const int wend = min(W, (q0 >> 6) + U);             // words [.., wend) are complete
            if ((wend & 63) == 0 || wend == W || (TILED && q0 + U * WAVE >= qEnd)) {   // flush the block of <= 64 words, coalesced (also at the end of a tile)
                const int wb = (wend - 1) & ~63;
                const int wlo = TILED ? max(R, c0 >> 6) : R;    // words in front of this tile were written when their tile was swept
#pragma unroll
                for (int x = 0; x < NR; ++x) {
                    const unsigned long long mreg = ((unsigned long long)mhi[x] << 32) | mlo[x];
                    if (r + x < nrows && wb + lane < wend && wb + lane >= wlo) mbase[(int64_t)k[x] * W + wb + lane] = mreg;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                        // table slices are rewritten by the next rows
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---------------------------------------------------------------------------------------------
// The same pair tests with CANDIDATE GENERATION in front of the exact gate (round 6).  Every reading of the gate needs
// |TA[i][i'] - TB[j][j']| < epsilon (the horizontal / full-length difference is one of its terms and the other is >= 0), and only
// ~3 % of the live pairs pass it.  What bounds the plain sweep is its two random f64 LDS gathers per 64 tests and row (one LDS per
// compute unit serves sixteen waves); a first prefilter that kept two gathers per row — 16-bit bins instead of doubles — was
// bit-identical and SLOWER (650 against 570 us per batch: profiles/r06).  Here a wave sweeps FOUR adjacent rows at once and the
// four rows' bins of one table column are ONE 8-byte LDS word: two 8-byte gathers per 64 columns serve 256 pair tests.  Bins are
// epsilon / 32 wide (15 bits; NaN entries and everything beyond the range share the last bin), compared as packed 16-bit halves;
// the survivors (~6 % of the columns) are compacted into a per-wave LDS queue, and the EXISTING exact f64 gate runs on the queue,
// 64 candidates at a time with every lane busy, its two table entries fetched from memory (L2) for those few and the two heights
// of the z gate from a per-object table in LDS (n1 + 1 + n2 doubles per workgroup, indexed like the bin table); a passing
// candidate sets its bit in the row's mask words in LDS (ds_or_b64), which go out coalesced at the end of the rows.
// The prefilter is a superset of the gate by construction: q(x) = trunc(min(x * invw, 32767)) is monotone, so |a - b| <= eps'
// gives |q(a) - q(b)| <= ceil(eps' * invw + rounding) <= 32 + 1; pre_K is 34.  A false positive (the last bin's far / NaN pairs
// included) costs an exact test, never a bit.  The exact gate sees the same operands in the same operation order as
// count_rows_lds: the mask words are bit-identical (tests/test_gpu_parity.py runs ladder cases, the ends of the bin range and
// the +-1-ulp plants through both kernels).
// ---------------------------------------------------------------------------------------------
constexpr int PRE_NR = 4;                 // rows a wave sweeps together (their bins share an LDS word)
constexpr int PRE_COLPAD = 128;           // sentinel columns behind the column tile (a sweep starts at the rows' own 64-column block and advances by 128)
constexpr int PRE_QCAP = 640;             // queue entries: the exact gate runs while 256 are waiting; a window's candidates go in at once when they fit (else 64 at a time)
constexpr int PRE_WAVES = 16;             // waves per workgroup of the prefiltered sweep (127 registers per lane: no spills; 12 waves measured 7 % slower)
// per-wave LDS of the prefiltered sweep: PRE_NR mask rows (TC / 64 words), the packed bin table (n1 + 1 + n2 entries of 8 bytes, ldsPerRow
// rounded), the queue (16-bit entries), the rows' own data (4 x 32 bytes)
__host__ __device__ constexpr int count_pre_wave_bytes(int ldsPerRow, int TC)
{
    return PRE_NR * (TC >> 6) * 8 + ldsPerRow * 8 + PRE_QCAP * 2 + PRE_NR * 32;
}
struct PreRow { double zi, zj; uint32_t rowA, rowB, moff, krow; };   // heights of the row's objects; first entries of its two table rows; byte offset of its mask words; the live row
typedef short pre_s2 __attribute__((ext_vector_type(2)));

template <int GM>
__device__ __forceinline__ void count_rows_pre(const DevParams& D, const ProbDesc& pd, int L, int row0, int nrows,
                                               uint32_t* qctr /* LDS: next quad of rows to hand out (0 on entry) */, int lane,
                                               const uint32_t* cIJ /* i_q | (n1 + 1 + j_q) << 16: table-slice indices; sentinel columns up to ((L + 127) & ~127) + 128 */,
                                               const double* __restrict__ TA, const double* __restrict__ TB,
                                               const uint16_t* __restrict__ QA, const uint16_t* __restrict__ QB /* the tables as bins (k_tables): rows of (n + 3 & ~3) entries */,
                                               uint2* qT /* n1 + 1 + n2 packed bin entries */, uint16_t* queue,
                                               unsigned long long* rmask /* PRE_NR rows of Wcap words, zero on entry and on exit */, int Wcap,
                                               PreRow* rowinfo,
                                               unsigned long long* __restrict__ mbase,
                                               const double* __restrict__ gZa, const double* __restrict__ gZb,
                                               const double* zT /* LDS, or NULL (no room: gZa / gZb serve instead): the objects' heights, indexed like the packed bin table */,
                                               uint32_t* degS /* LDS, or NULL: the full degree of every live row, counted as the pairs pass (whole problems only) */)
{
    constexpr int NR = PRE_NR;
    const int W = (L + 63) >> 6;
    const int Lpad = (L + 2 * WAVE - 1) & ~(2 * WAVE - 1);
    const uint32_t K2 = (uint32_t)D.pre_K * 0x00010001u;
    const int n1 = pd.n1, n2 = pd.n2;
    const int nq1 = (n1 + 3) & ~3, nq2 = (n2 + 3) & ~3;
    const bool pre = n1 <= 4 * WAVE && n2 <= 4 * WAVE;         // a lane holds four consecutive entries of a row: one 8-byte load per row
    uint2 ra[NR], rb[NR];
    int pi[NR], pj[NR];                                         // objects of the rows whose bin rows are in ra / rb
    double pzi = 0.0, pzj = 0.0;                                // lane x < NR: the heights of row x's two objects
    auto fetch_z = [&](int r_) {                                // (the live row's own entries of the pools are its objects' heights: the same bits either way)
        if (!GM) return;
        const int kz_ = row0 + min(r_ + min(lane, NR - 1), nrows - 1);
        if (zT != nullptr) { const uint32_t pk_ = cIJ[kz_]; pzi = zT[pk_ & 0xffffu]; pzj = zT[pk_ >> 16]; }
        else { pzi = gZa[kz_]; pzj = gZb[kz_]; }
    };
    auto fetch_tab = [&](int r_) {
        fetch_z(r_);
#pragma unroll
        for (int x = 0; x < NR; ++x) {
            const int k_ = row0 + min(r_ + x, nrows - 1);
            const uint32_t pk_ = cIJ[k_];
            pi[x] = __builtin_amdgcn_readfirstlane((int)(pk_ & 0xffffu)); pj[x] = __builtin_amdgcn_readfirstlane((int)(pk_ >> 16) - (n1 + 1));
            ra[x] = *reinterpret_cast<const uint2*>(QA + (int64_t)pi[x] * nq1 + min(4 * lane, nq1 - 4));
            rb[x] = *reinterpret_cast<const uint2*>(QB + (int64_t)pj[x] * nq2 + min(4 * lane, nq2 - 4));
        }
    };
    // Quads of rows are handed out in order (an LDS counter): the rows in front sweep the most columns, so the longest quads start
    // first and the waves of a workgroup finish within one quad of each other whatever their number
    auto grab = [&]() -> int {
        uint32_t g = 0u;
        if (lane == 0) g = __hip_atomic_fetch_add(qctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return NR * __builtin_amdgcn_readfirstlane((int)g);
    };
    int r = grab(), rnext = nrows;
    if (pre && r < nrows) fetch_tab(r);
    uint32_t qn = 0;                                            // queue fill (wave-uniform)
#ifdef ROMAN_COUNT_TIMING
    unsigned long long tc_[6] = {0, 0, 0, 0, 0, 0}; unsigned long long tm_; unsigned nq_ = 0, ncons_ = 0, npush_ = 0;   // stage, sweep, push, consume, store, (unused)
#define TCK(k_) do { const unsigned long long n_ = __builtin_readcyclecounter(); tc_[k_] += n_ - tm_; tm_ = n_; } while (0)
#else
#define TCK(k_) do { } while (0)
#endif
    auto lds_order = [&]() {                                    // LDS operations of one wave execute in order: this is for the compiler
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // The exact gate over up to 256 queue entries starting at `base`: four candidates per lane, the operands of all four requested
    // (table entries from memory: L2; heights from the per-object table in LDS, or from memory where the launch had no room for it)
    // before the first is used — a single chain's round trip would otherwise be all a wave does
    auto consume = [&](uint32_t base, uint32_t n) {
        constexpr int CH = 4;
        uint32_t e[CH]; double a[CH], bb[CH], za[CH], zb[CH];
        auto gather = [&](auto zlds_) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const uint32_t idx = (uint32_t)(c * WAVE + lane);
                e[c] = idx < n ? (uint32_t)queue[base + idx] : 0xffffu;     // (0x3fff: a column beyond every live set: inactive below)
                const uint32_t qq = e[c] & 0x3fffu;
                const bool act = (int)qq < L;                   // (a sentinel column can only get here through the last bin)
                const uint32_t pk = cIJ[act ? qq : 0u];
                const PreRow* ri = rowinfo + (e[c] >> 14);
                a[c] = TA[ri->rowA + (pk & 0xffffu)];           // (32-bit element offsets: maps of at most 32767 objects take this sweep)
                bb[c] = TB[ri->rowB + (pk >> 16)];              // (rowB is short of the row's start by n1 + 1: the packed index carries it)
                if (GM) {
                    if (decltype(zlds_)::value) { za[c] = zT[pk & 0xffffu]; zb[c] = zT[pk >> 16]; }
                    else { za[c] = gZa[act ? qq : 0u]; zb[c] = gZb[act ? qq : 0u]; }
                }
            }
        };
        if (GM && zT != nullptr) gather(std::true_type()); else gather(std::false_type());      // (wave-uniform: the launch's choice)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t qq = e[c] & 0x3fffu, x = e[c] >> 14;
            double dz = 0.0;
            if (GM) { const PreRow* ri = rowinfo + x; dz = fabs((ri->zi - za[c]) - (ri->zj - zb[c])); }
            const bool is = (int)qq < L && pair_gate<GM>(D, a[c], bb[c], dz);
            if (is) {
                const PreRow* ri = rowinfo + x;
                (void)__hip_atomic_fetch_or(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(rmask) + ri->moff + ((qq >> 6) << 3)),
                                            1ull << (qq & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // a pair of the strict upper triangle counts for both of its rows (k_lists' degrees: it then skips its own sweep)
                if (degS != nullptr && qq > ri->krow) {
                    (void)__hip_atomic_fetch_add(degS + ri->krow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    (void)__hip_atomic_fetch_add(degS + qq, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    };
    // candidate bits of a window (up to four steps of two 64-column chunks: bit 8 s + 4 t + x of a lane = column qwin + (2 s + t) 64 + lane,
    // row x) -> queue entries; the exact gate runs whenever 256 entries are waiting
    auto flush = [&](uint32_t acc, int qwin) {
        const uint32_t cnt = (uint32_t)__builtin_popcount(acc);
        const uint32_t incl = wave_incl_scan(cnt);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t qb = (uint32_t)(qwin + lane);
        if (qn + total <= (uint32_t)PRE_QCAP) {
            // the usual case: every lane writes its own candidates behind those of the lanes in front of it (one scan, no ballots)
            uint32_t at = qn + incl - cnt;
            while (__ballot(acc != 0u) != 0ull) {
                if (acc != 0u) {
                    const uint32_t b = (uint32_t)__builtin_ctz(acc);
                    acc &= acc - 1u;
                    queue[at++] = (uint16_t)((qb + ((b >> 2) << 6)) | ((b & 3u) << 14));
                }
#ifdef ROMAN_COUNT_TIMING
                ++npush_;
#endif
            }
            qn += total;
        } else {
            // a window with more candidates than the queue has room for: 64 at a time, the exact gate in between
            while (true) {
                const unsigned long long m = __ballot(acc != 0u);
                if (m == 0ull) break;
                const uint32_t b = (uint32_t)__builtin_ctz(acc | 0x80000000u);
                const bool has = acc != 0u;
                acc &= acc - 1u;
                const uint32_t at = qn + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (has) queue[at] = (uint16_t)((qb + ((b >> 2) << 6)) | ((b & 3u) << 14));
                qn += (uint32_t)__popcll(m);
                if (qn >= 256u) { TCK(2); lds_order(); qn -= 256u; consume(qn, 256u); lds_order(); TCK(3); }
            }
        }
        if (qn >= 256u) {
            TCK(2); lds_order();
            while (qn >= 256u) { qn -= 256u; consume(qn, 256u);
#ifdef ROMAN_COUNT_TIMING
                ++ncons_;
#endif
            }
            lds_order(); TCK(3);
        }
    };
    for (; r < nrows; r = rnext) {
#ifdef ROMAN_COUNT_TIMING
        tm_ = __builtin_readcyclecounter(); ++nq_;
#endif
        int k[NR];
#pragma unroll
        for (int x = 0; x < NR; ++x) k[x] = __builtin_amdgcn_readfirstlane(row0 + min(r + x, nrows - 1));
        if (!pre) {
#pragma unroll
            for (int x = 0; x < NR; ++x) {
                const uint32_t pk_ = cIJ[k[x]];
                pi[x] = __builtin_amdgcn_readfirstlane((int)(pk_ & 0xffffu)); pj[x] = __builtin_amdgcn_readfirstlane((int)(pk_ >> 16) - (n1 + 1));
            }
        }
        if (!pre) fetch_z(r);
        if (lane < NR) {                                        // the rows' own objects and heights, for the exact gate
            int i_ = pi[0], j_ = pj[0];
#pragma unroll
            for (int x = 1; x < NR; ++x) if (lane == x) { i_ = pi[x]; j_ = pj[x]; }
            PreRow ri; ri.rowA = (uint32_t)i_ * (uint32_t)n1; ri.rowB = (uint32_t)j_ * (uint32_t)n2 - (uint32_t)(n1 + 1);
            ri.moff = (uint32_t)lane * (uint32_t)Wcap * 8u; ri.zi = pzi; ri.zj = pzj;
            int kr_ = k[0];
#pragma unroll
            for (int x = 1; x < NR; ++x) if (lane == x) kr_ = (r + x < nrows) ? k[x] : 0x7fffffff;   // (a duplicated last row counts nothing)
            ri.krow = (uint32_t)kr_;
            rowinfo[lane] = ri;
        }
        // the packed bin table: entry t = the NR rows' bins of table column t (map-1 columns, the sentinel, map-2 columns)
        if (pre) {
            // lane l holds entries 4 l .. 4 l + 3 of every row: the low / high halves of its two words, zipped over the rows
            const int t0 = 4 * lane;
            if (t0 < n1) qT[t0] = make_uint2(__builtin_amdgcn_perm(ra[1].x, ra[0].x, 0x05040100u), __builtin_amdgcn_perm(ra[3].x, ra[2].x, 0x05040100u));
            if (t0 + 1 < n1) qT[t0 + 1] = make_uint2(__builtin_amdgcn_perm(ra[1].x, ra[0].x, 0x07060302u), __builtin_amdgcn_perm(ra[3].x, ra[2].x, 0x07060302u));
            if (t0 + 2 < n1) qT[t0 + 2] = make_uint2(__builtin_amdgcn_perm(ra[1].y, ra[0].y, 0x05040100u), __builtin_amdgcn_perm(ra[3].y, ra[2].y, 0x05040100u));
            if (t0 + 3 < n1) qT[t0 + 3] = make_uint2(__builtin_amdgcn_perm(ra[1].y, ra[0].y, 0x07060302u), __builtin_amdgcn_perm(ra[3].y, ra[2].y, 0x07060302u));
            uint2* qB = qT + n1 + 1;
            if (t0 < n2) qB[t0] = make_uint2(__builtin_amdgcn_perm(rb[1].x, rb[0].x, 0x05040100u), __builtin_amdgcn_perm(rb[3].x, rb[2].x, 0x05040100u));
            if (t0 + 1 < n2) qB[t0 + 1] = make_uint2(__builtin_amdgcn_perm(rb[1].x, rb[0].x, 0x07060302u), __builtin_amdgcn_perm(rb[3].x, rb[2].x, 0x07060302u));
            if (t0 + 2 < n2) qB[t0 + 2] = make_uint2(__builtin_amdgcn_perm(rb[1].y, rb[0].y, 0x05040100u), __builtin_amdgcn_perm(rb[3].y, rb[2].y, 0x05040100u));
            if (t0 + 3 < n2) qB[t0 + 3] = make_uint2(__builtin_amdgcn_perm(rb[1].y, rb[0].y, 0x07060302u), __builtin_amdgcn_perm(rb[3].y, rb[2].y, 0x07060302u));
        } else {
            for (int t = lane; t < n1; t += WAVE) {
                uint32_t b_[NR];
#pragma unroll
                for (int x = 0; x < NR; ++x) b_[x] = QA[(int64_t)pi[x] * nq1 + t];
                qT[t] = make_uint2(b_[0] | (b_[1] << 16), b_[2] | (b_[3] << 16));
            }
            for (int t = lane; t < n2; t += WAVE) {
                uint32_t b_[NR];
#pragma unroll
                for (int x = 0; x < NR; ++x) b_[x] = QB[(int64_t)pj[x] * nq2 + t];
                qT[n1 + 1 + t] = make_uint2(b_[0] | (b_[1] << 16), b_[2] | (b_[3] << 16));
            }
        }
        if (lane == 0) qT[n1] = make_uint2(0x7fff7fffu, 0x7fff7fffu);   // sentinel entry of the padding columns
        lds_order();
        rnext = grab();
        if (pre && rnext < nrows) fetch_tab(rnext);

        TCK(0);
        const int R = k[0] >> 6;                                // the NR rows of a wave lie in the same 64-row block
        const char* qbytes = reinterpret_cast<const char*>(qT);
        uint32_t nacc = 0u;                                     // NOT-candidate bits of the current window
        int step = 0, qwin = R << 6;
        for (int q0 = R << 6; q0 < Lpad; q0 += 2 * WAVE, ++step) {
            uint32_t pk[2]; uint2 ea[2], eb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) pk[t] = cIJ[q0 + t * WAVE + lane];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                ea[t] = *reinterpret_cast<const uint2*>(qbytes + ((pk[t] & 0xffffu) << 3));
                eb[t] = *reinterpret_cast<const uint2*>(qbytes + ((pk[t] >> 16) << 3));
            }
            uint32_t n8 = 0u;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                // per 16-bit half: K - |a - b| is negative (sign bit set) where the pair is NOT a candidate
                const pre_s2 c0 = __builtin_bit_cast(pre_s2, K2) - __builtin_elementwise_abs(__builtin_bit_cast(pre_s2, ea[t].x) - __builtin_bit_cast(pre_s2, eb[t].x));
                const pre_s2 c1 = __builtin_bit_cast(pre_s2, K2) - __builtin_elementwise_abs(__builtin_bit_cast(pre_s2, ea[t].y) - __builtin_bit_cast(pre_s2, eb[t].y));
                const uint32_t u = ((__builtin_bit_cast(uint32_t, c0) & 0x80008000u) >> 15) | ((__builtin_bit_cast(uint32_t, c1) & 0x80008000u) >> 13);
                n8 |= ((u | (u >> 15)) & 0xfu) << (4 * t);      // row 0 -> bit 0, row 1 (bit 16) -> bit 1, row 2 -> bit 2, row 3 (bit 18) -> bit 3
            }
            nacc |= n8 << ((step & 3) << 3);
            if ((step & 3) == 3) {
                TCK(1);
                flush(~nacc, qwin);
                TCK(2);
                nacc = 0u; qwin = q0 + 2 * WAVE;
            }
        }
        TCK(1);
        if (step & 3) flush(~nacc & ((1u << ((step & 3) << 3)) - 1u), qwin);
        TCK(2);
        lds_order();
        if (qn) { consume(0u, qn); qn = 0u; }
        lds_order();
        TCK(3);
        // the rows' words [R, W): out, coalesced, and cleared for the next rows
#pragma unroll
        for (int x = 0; x < NR; ++x) {
            for (int wv = R + lane; wv < W; wv += WAVE) {
                const unsigned long long mreg = rmask[x * Wcap + wv];
                rmask[x * Wcap + wv] = 0ull;
                // (non-temporal: the mask rows are read next by another kernel, from whatever XCD; measured -5 us here, -3 us in k_lists)
                if (r + x < nrows) __builtin_nontemporal_store(mreg, &mbase[(int64_t)k[x] * W + wv]);
            }
        }
        lds_order();                                            // the bin table and the rows' data are rewritten by the next rows
        TCK(4);
    }
#ifdef ROMAN_COUNT_TIMING
    if (lane == 0 && (threadIdx.x >> 6) == 0 && (blockIdx.x & 63) == 0 && row0 == 0 && nq_ > 0)
        printf("[k_count pre] wg %d L %d quads %u: stage %llu sweep %llu push %llu (iterations %u) consume %llu (+%u inside the sweep) store %llu cycles per quad\n", (int)blockIdx.x, L, nq_,
               tc_[0] / nq_, tc_[1] / nq_, tc_[2] / nq_, npush_ / nq_, tc_[3] / nq_, ncons_, tc_[4] / nq_);
#endif
#undef TCK
}

// A work item of a live set that does not fit the LDS column tile (no semantic gate: L = n1 * n2): the item's rows are swept
// against one tile of columns after the other (a row needs only the words at and behind its own 64-row block: the tiles in
// front of the item's first row are skipped).  Its own kernel instantiation (k_count<..., true>): the one-tile kernel keeps the code it had.
template <int GM, int NR>
__device__ __forceinline__ void count_item_tiled(const DevParams& D, const ProbDesc& pd, int L, int row0, int nrows,
                                              uint32_t* cIJ, double2* cZZ, const double* __restrict__ TA, const double* __restrict__ TB,
                                              double* tA, int ldsPerRow, unsigned long long* __restrict__ mbase, int TC,
                                              const int32_t* __restrict__ gI, const int32_t* __restrict__ gJ,
                                              const double* __restrict__ gZa, const double* __restrict__ gZb)
{
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = uni_i(tid >> 6), wpb = nt >> 6;
    L = uni_i(L); row0 = uni_i(row0); nrows = uni_i(nrows); TC = uni_i(TC); ldsPerRow = uni_i(ldsPerRow);   // (wave-uniform: back into scalar registers)
    const int Lpad = (L + 255) & ~255;
    for (int c0 = (((row0 >> 6) << 6) / TC) * TC; c0 < Lpad; c0 += TC) {
        const int clen = min(TC, Lpad - c0);
        __syncthreads();                        // every wave is done with the previous tile's columns
        for (int q = tid; q < clen; q += nt) {
            const int qq = c0 + q;
            const bool v = qq < L;
            cIJ[q] = v ? ((uint32_t)gI[qq] | ((uint32_t)(pd.n1 + 1 + gJ[qq]) << 16)) : ((uint32_t)pd.n1 | ((uint32_t)(pd.n1 + 1) << 16));
            if (GM) cZZ[q] = v ? make_double2(gZa[qq], gZb[qq]) : make_double2(0.0, 0.0);
        }
        __syncthreads();
        count_rows_lds<GM, NR, true>(D, pd, L, row0, nrows, w, wpb, lane, cIJ, cZZ, TA, TB, tA, ldsPerRow, mbase, c0, clen, gI, gJ, gZa, gZb);
    }
}

template <int GM, int NR, bool TILED, bool PRE = false /* candidate generation in front of the exact gate (one-tile sweep only): count_rows_pre */>
__global__ void __launch_bounds__(PRE ? PRE_WAVES * 64 : 1024) k_count(DevParams D, const ProbDesc* __restrict__ probs,
                                                const ProbState* __restrict__ st,
                                                const BatchTotals* __restrict__ tot,
                                                const ItemDesc* __restrict__ items,
                                                const double* __restrict__ tabPool,
                                                const int32_t* __restrict__ li, const int32_t* __restrict__ lj,
                                                const double* __restrict__ lza, const double* __restrict__ lzb,
                                                uint32_t* __restrict__ rowCnt,
                                                unsigned long long* __restrict__ maskPool,
                                                uint32_t* __restrict__ prefPool,
                                                int TC /* LDS column tile (multiple of 256) */, int ldsPerWave /* doubles: NR table slices */, int RPB,
                                                const uint16_t* __restrict__ qtabPool /* PRE: the tables as bins (k_tables) */,
                                                int zLds /* PRE, GM: the launch's LDS holds the height table (0: the exact gate reads lza / lzb) */)
{
    // LDS: [GM: cZZ[TC]] cIJ[TC] | per wave NR table slices (n1 + 1 + n2 doubles each)
    // PRE (NR is ignored: PRE_NR rows per wave; ldsPerWave = entries of the packed bin table): cIJ[TC + PRE_COLPAD] | counter | [whole
    // problems: degL[TC]] | [zLds: zT[ldsPerWave]] | per wave count_pre_wave_bytes()
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double2* cZZ = reinterpret_cast<double2*>(smem);
    uint32_t* cIJ = reinterpret_cast<uint32_t*>(cZZ + ((GM && !PRE) ? TC : 0));
    double* tabs = reinterpret_cast<double*>(cIJ + TC);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, w = tid >> 6, wpb = nt >> 6;
    double* tA = tabs + (size_t)w * ldsPerWave;
    // (PRE) no f64 table slices at all: per wave the mask rows, the packed bin table, the queue, the rows' data
    const int preBytes = PRE ? count_pre_wave_bytes(ldsPerWave, TC) : 0;
    uint32_t* qctr = cIJ + TC + PRE_COLPAD;                      // (PRE) the rows' hand-out counter, 16 bytes
    uint32_t* degL = cIJ + TC + PRE_COLPAD + 4;                  // (PRE, whole problems) TC row degrees
    // (PRE with the z gate, when the launch has the room: zLds != 0) the objects' heights, ldsPerWave doubles indexed like the packed bin table
    double* zT = reinterpret_cast<double*>(cIJ + TC + PRE_COLPAD + 4 + ((PRE && RPB < 0) ? TC : 0));
    const bool zInLds = PRE && GM && zLds != 0;
    unsigned char* pw = reinterpret_cast<unsigned char*>(zT + (zInLds ? ldsPerWave : 0)) + (size_t)w * preBytes;
    unsigned long long* rmask = reinterpret_cast<unsigned long long*>(pw);
    uint2* qT = reinterpret_cast<uint2*>(rmask + PRE_NR * (TC >> 6));
    uint16_t* queue = reinterpret_cast<uint16_t*>(qT + ldsPerWave);
    PreRow* rowinfo = reinterpret_cast<PreRow*>(queue + PRE_QCAP);
    if (PRE) { for (int x = lane; x < PRE_NR * (TC >> 6); x += WAVE) rmask[x] = 0ull; }
    // PRE with RPB < 0: a work item is a whole PROBLEM (B = -RPB problems; batches with at least a problem per compute unit): the
    // column tile is staged once per problem instead of once per 128 rows, and the rows go to the waves quad by quad
    const bool whole = PRE && RPB < 0;
    const int nItems = whole ? -RPB : tot->items;
    // XCD-aware order (workgroup ids are dealt to the 8 XCDs round-robin): XCD x takes the CONTIGUOUS range [x Gx, (x + 1) Gx) of
    // work items — the items of a problem, which share its tables, columns and mask rows, run on one L2
    const int Gx_ = (nItems + 7) >> 3;
    for (int sIdx_ = blockIdx.x; (sIdx_ >> 3) < Gx_; sIdx_ += gridDim.x) {
        // (whole problems: problem t on the XCD t mod 8, where k_lists — one workgroup per problem, b = blockIdx — reads its mask rows)
        const int t = whole ? sIdx_ : (sIdx_ & 7) * Gx_ + (sIdx_ >> 3);
        if (t >= nItems) continue;
        ItemDesc it;
        if (whole) { it.b = t; it.row0 = 0; if (st[t].kind >= 2 || st[t].L <= 0) continue; } else it = items[t];
        const int b = it.b;
        const ProbDesc pd = probs[b];
        const int L = st[b].L;
        const int64_t lo = pd.liveOff, mo = st[b].maskOff;
        const int nrows = whole ? L : min(RPB, L - it.row0);
        const double* TA = tabPool + pd.tabOff;
        const double* TB = TA + (int64_t)pd.n1 * pd.n1;
        const int Lpad = (L + 255) & ~255;
        // The column data of the whole live set in LDS when it fits (the usual case); a larger live set (no semantic gate:
        // L = n1 * n2) is swept TILE BY TILE — the item's rows are staged once per tile (a row needs only the words at and
        // behind its own 64-row block: tiles in front of the item's first row are skipped).
        // TILED == false: the items whose whole live set fits the LDS column tile (the usual case: one sweep per row);
        // TILED == true (a second launch, only when such problems can exist): the others, tile by tile.
        if ((Lpad <= TC) == TILED) continue;
        if (!TILED) {
            __syncthreads();                    // every wave is done with the previous item's columns
            for (int q = tid; q < Lpad + (PRE ? PRE_COLPAD : 0); q += nt) {     // (PRE: sentinel columns up to the end of a sweep's last step)
                const bool v = q < L;
                cIJ[q] = v ? ((uint32_t)li[lo + q] | ((uint32_t)(pd.n1 + 1 + lj[lo + q]) << 16)) : ((uint32_t)pd.n1 | ((uint32_t)(pd.n1 + 1) << 16));
                if (GM && !PRE) cZZ[q] = v ? make_double2(lza[lo + q], lzb[lo + q]) : make_double2(0.0, 0.0);
                // (PRE) the heights per OBJECT: every live column writes its two objects' entries — columns that share an object store
                // the same bits (k_live copied them from the object's features), and an object of no live column is never looked up
                if (zInLds && v) { zT[li[lo + q]] = lza[lo + q]; zT[pd.n1 + 1 + lj[lo + q]] = lzb[lo + q]; }
            }
            if (zInLds && tid == 0) zT[pd.n1] = 0.0;             // (the sentinel columns' entry)
            if (PRE && tid == 0) *qctr = 0u;
            if (PRE && whole) for (int q = tid; q < L; q += nt) degL[q] = 0u;
            __syncthreads();
            if (PRE) {
                count_rows_pre<GM>(D, pd, L, it.row0, nrows, qctr, lane, cIJ, TA, TB,
                                   qtabPool + 4 * (int64_t)pd.qtabOff4, qtabPool + 4 * (int64_t)pd.qtabOff4 + (int64_t)pd.n1 * ((pd.n1 + 3) & ~3),
                                   qT, queue, rmask, TC >> 6, rowinfo, maskPool + mo, lza + lo, lzb + lo, zInLds ? zT : nullptr, whole ? degL : nullptr);
                if (whole) {                                    // the problem's degrees, for k_lists (live order)
                    __syncthreads();
                    for (int q = tid; q < L; q += nt) rowCnt[lo + q] = degL[q];
                }
            }
            else
            count_rows_lds<GM, NR, false>(D, pd, L, it.row0, nrows, w, wpb, lane, cIJ, cZZ, TA, TB, tA, ldsPerWave / NR, maskPool + mo,
                                          0, Lpad, li + lo, lj + lo, lza + lo, lzb + lo);
        } else {
            count_item_tiled<GM, NR>(D, pd, L, it.row0, nrows, cIJ, cZZ, TA, TB, tA, ldsPerWave / NR, maskPool + mo, TC,
                                     li + lo, lj + lo, lza + lo, lzb + lo);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_mirror: lower triangle of the candidate bit matrix.  Block (c, R) of 64x64 bits, c > R, is the
// transpose of block (R, c) that k_count produced: lane l loads word c of row R*64+l, the wave
// transposes the 64x64 bit block in registers (6 butterfly stages) and lane l stores word R of row
// c*64+l.  (The earlier scheme, one 8-byte atomic OR per hit from inside k_count, cost 0.25 ms per
// batch of 256; this kernel takes 0.13 ms and needs no zeroed mask pool.)
// A wave owns 1 x 8 blocks: it loads the words c..c+7 of the 64 rows of source row block R (one cache line per
// row for all 8 loads, all in flight together).  The 8 waves of a workgroup take 8 consecutive R for the same
// c range: their stores to words R..R+7 of a target row fall into one line and are merged by the write-back L2.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long transpose64(unsigned long long x, int lane)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long m = (s == 32) ? 0x00000000ffffffffull : (s == 16) ? 0x0000ffff0000ffffull : (s == 8) ? 0x00ff00ff00ff00ffull
                                   : (s == 4) ? 0x0f0f0f0f0f0f0f0full : (s == 2) ? 0x3333333333333333ull : 0x5555555555555555ull;
        const unsigned long long o = __shfl_xor(x, s);
        x = (lane & s) ? ((x & ~m) | ((o & ~m) >> s)) : ((x & m) | ((o & m) << s));
    }
    return x;
}

__global__ void __launch_bounds__(512) k_mirror(int B, int T /* workgroups per problem */, const ProbState* __restrict__ st, unsigned long long* __restrict__ maskPool, int skip0)
{
    // The bit matrices are SPARSE (1.8 set bits per 64-bit word at config 3): a block is transposed by scattering its set
    // bits — lane l (source row) ORs bit l into word j of the wave's LDS tile for every set bit j of its word, one LDS atomic
    // per set bit — instead of the dense 6-stage butterfly (transpose64: ~130 instructions per block whatever it holds;
    // this kernel was bound by them, 153 us per batch of 256).  LDS operations of one wave execute in order: no barriers.
    __shared__ unsigned long long tile[8][8][64];                 // per wave: 8 blocks x 64 target words
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    // All T workgroups of a problem carry ids that are congruent modulo 8: one XCD, one L2 (k_cos).  A 128-byte line of the
    // lower triangle collects its 16 words from 16 different tasks; dealt round-robin over the 8 non-coherent L2s every one
    // of them wrote its part of the line back separately (2.2 x the bytes, read-modify-write in HBM: half this kernel's time).
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int b = (slot / T) * 8 + xcd, tb = slot % T;
    if (b >= B) return;
    if (st[b].kind >= 2 || (skip0 && st[b].kind == 0)) return;    // (skip0: the stream-layout problems take k_lists — no symmetric matrix needed)
    const int L = st[b].L;
    const int W = (L + 63) >> 6;
    const int nR = ((W - 1 + nw - 1) / nw) * nw;                  // source row blocks 0..W-2, padded to whole workgroups
    const int nTasks = ((W + 7) / 8) * max(nR, 1);                // (column strip of 8 words) x (source row block)
    unsigned long long* mb = maskPool + st[b].maskOff;
    // the grid was sized from an ESTIMATE of the largest live set: a larger problem takes several rounds
    for (int task = tb * nw + w; task < nTasks; task += T * nw) {
        const int ct = task / max(nR, 1), R = task - ct * nR;
        const int cb = ct * 8;
        if (R >= W - 1 || cb >= W || cb + 7 <= R) continue;       // nothing below the diagonal in this strip
        const unsigned long long* src = mb + (int64_t)(R * 64 + lane) * W;         // rows R*64+lane < (W-1)*64 < L exist
        unsigned long long x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (cb + i > R && cb + i < W) ? src[cb + i] : 0ull;
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[w][i][lane] = 0ull;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const unsigned long long me = 1ull << lane;
        for (;;) {
            unsigned long long left = 0ull;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (x[i]) {
                    const int j = __builtin_ctzll(x[i]);
                    (void)__hip_atomic_fetch_or(&tile[w][i][j], me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    x[i] &= x[i] - 1ull;
                }
                left |= x[i];
            }
            if (__ballot(left != 0ull) == 0ull) break;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = cb + i;
            if (c > R && c < W) {                                // wave-uniform
                const unsigned long long y = tile[w][i][lane];
                if (c * 64 + lane < L) mb[(int64_t)(c * 64 + lane) * W + R] = y;
            }
        }
        __builtin_amdgcn_wave_barrier();                         // (the next task zeroes the tile behind these reads: in order)
    }
}

// ---------------------------------------------------------------------------------------------
// k_rowprefix: per live row, the number of candidates in front of every 64-column mask word (the entry
// index of the word's first candidate in k_fill) and the row total.  One wave per row, lanes = words.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_rowprefix(const ProbDesc* __restrict__ probs, const ProbState* __restrict__ st,
                                                    const BatchTotals* __restrict__ tot, const ItemDesc* __restrict__ items,
                                                    const unsigned long long* __restrict__ maskPool, uint32_t* __restrict__ prefPool,
                                                    uint32_t* __restrict__ rowCnt, int RPB, int skip0 /* stream-layout problems take k_lists */)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int nItems = tot->items;
    // XCD-aware order (workgroup ids are dealt to the 8 XCDs round-robin): XCD x takes the CONTIGUOUS range [x Gx, (x + 1) Gx) of
    // work items — the items of a problem, which share its tables, columns and mask rows, run on one L2
    const int Gx_ = (nItems + 7) >> 3;
    for (int sIdx_ = blockIdx.x; (sIdx_ >> 3) < Gx_; sIdx_ += gridDim.x) {
        const int t = (sIdx_ & 7) * Gx_ + (sIdx_ >> 3);
        if (t >= nItems) continue;
        const ItemDesc it = items[t];
        const int b = it.b;
        const int L = st[b].L;
        const int W = (L + 63) >> 6;
        const int64_t lo = probs[b].liveOff, mo = st[b].maskOff;
        const int nrows = min(RPB, L - it.row0);
        const bool wantPrefix = st[b].kind != 0;               // the stream layout takes its prefix counts in k_upper
        if (skip0 && !wantPrefix) continue;
        if (W <= WAVE) {                                        // one word per lane: four rows per step, their loads in flight together
            constexpr int U = 4;
            for (int r = w; r < nrows; r += U * wpb) {
                uint32_t c[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = it.row0 + min(r + u * wpb, nrows - 1);
                    c[u] = (lane < W) ? (uint32_t)__popcll(maskPool[mo + (int64_t)k * W + lane]) : 0u;
                }
                uint32_t inc[U];
#pragma unroll
                for (int u = 0; u < U; ++u) inc[u] = wave_incl_scan(c[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (r + u * wpb < nrows) {
                        const int k = it.row0 + r + u * wpb;
                        if (wantPrefix && lane < W) prefPool[mo + (int64_t)k * W + lane] = inc[u] - c[u];
                        if (lane == WAVE - 1) rowCnt[lo + k] = inc[u];
                    }
                }
            }
            continue;
        }
        for (int r = w; r < nrows; r += wpb) {
            const int k = it.row0 + r;
            const unsigned long long* mrow = maskPool + mo + (int64_t)k * W;
            uint32_t* prow = prefPool + mo + (int64_t)k * W;
            uint32_t carry = 0;
            for (int wb = 0; wb < W; wb += WAVE) {
                const bool v = wb + lane < W;
                const uint32_t c = v ? (uint32_t)__popcll(mrow[wb + lane]) : 0u;
                const uint32_t ex = wave_excl_scan(c, lane);
                if (v && wantPrefix) prow[wb + lane] = carry + ex;
                carry += __shfl(ex + c, WAVE - 1);
            }
            if (lane == 0) rowCnt[lo + k] = carry;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_rowsort: per problem, the live rows ordered by descending candidate count (degree).
//  kind 0 (stream layout): a STABLE, deterministic order — rank(k) = #{rows with a larger degree} + #{rows k' < k with
//    the same degree} — because the rank becomes the association's POSITION, the numbering of the stored matrix
//    (which entries a row keeps).  Bitonic sort of unique (degree, row) keys in LDS.  Slice geometry follows in
//    k_slicegeom, once k_upper knows the upper degrees.
//  kind 1 (fallback): counting sort with atomic ranks (the order among rows of equal degree is arbitrary — it
//    changes where a row is stored, never what is computed for it), then the sorted SELL-64 geometry:
//    rowPos[k] = sorted position of row k, perm[pos] = row, per slice its width (longest row) and base offset.
// ---------------------------------------------------------------------------------------------
// Positions of the stream layout WITHOUT a sort.  The position of row k is its rank by (degree descending, row ascending):
//   #(rows of larger degree) + #(rows of the same degree and smaller index).
// Degrees are small integers: a histogram (LDS atomics), its scan in descending degree order (= where every degree's range of
// positions starts), a scatter of the rows into their degree's range in whatever order the atomics grant, and the rank of a row inside
// its range by counting the smaller row indices there (a dozen rows share a degree on average).  keys[0 .. L) receives what the
// bitonic sort of the unique keys ((degree + 1) << 12) | (4095 - row) left there — the same array, bit for bit — and zeros up to N.
// The bitonic sort it stands for was 67 k cycles of k_lists' 390 k per problem and 30 us of the single-pair call (k_rowsort).
// Returns false (nothing written that matters) when more than eqMax rows share one degree — the ranks inside a range cost its
// square —: the caller sorts.  deg(k): degree of live row k (< L).  wsum: nt / 64 + 2 words.
template <class DegF>
__device__ __forceinline__ bool place_keys(int L, int N, int eqMax, DegF deg, uint32_t* keys, uint32_t* hcnt /* [L] */, uint32_t* hcur /* [L] */,
                                           uint16_t* tmp /* [L] */, uint32_t* wsum)
{
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6, nw = nt >> 6;
    for (int d = tid; d < L; d += nt) hcnt[d] = 0u;
    if (tid == 0) { wsum[nw] = 0u; wsum[nw + 1] = 0u; }           // carry of the scan, largest group of equal degrees
    __syncthreads();
    for (int k = tid; k < L; k += nt) atomicAdd(&hcnt[deg(k)], 1u);
    __syncthreads();
    uint32_t mx = 0u;
    for (int r0 = 0; r0 < L; r0 += nt) {                           // exclusive scan over the bins, LARGEST degree first
        const int r = r0 + tid;
        const uint32_t v = r < L ? hcnt[L - 1 - r] : 0u;
        mx = max(mx, v);
        const uint32_t inc = wave_incl_scan(v);
        if (lane == WAVE - 1) wsum[w] = inc;
        __syncthreads();
        uint32_t wbase = 0u, tot = 0u;
        for (int t = 0; t < nw; ++t) { if (t < w) wbase += wsum[t]; tot += wsum[t]; }
        const uint32_t carry = wsum[nw];
        if (r < L) hcur[L - 1 - r] = carry + wbase + inc - v;
        __syncthreads();
        if (tid == 0) wsum[nw] = carry + tot;
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    if (lane == 0) atomicMax(&wsum[nw + 1], mx);
    __syncthreads();
    if ((int)wsum[nw + 1] > eqMax) return false;                   // (the same word in every thread)
    for (int k = tid; k < L; k += nt) { const uint32_t slot = atomicAdd(&hcur[deg(k)], 1u); tmp[slot] = (uint16_t)k; }   // hcur[d] ends as the END of d's range
    for (int t = L + tid; t < N; t += nt) keys[t] = 0u;
    __syncthreads();
    for (int i = tid; i < L; i += nt) {
        const uint32_t k = tmp[i], d = (uint32_t)deg((int)k);
        const uint32_t end = hcur[d], start = end - hcnt[d];
        uint32_t r = 0u;
        for (uint32_t j = start; j < end; j += 4u) {
            uint32_t o[4];
#pragma unroll
            for (uint32_t x = 0; x < 4u; ++x) o[x] = tmp[min(j + x, end - 1u)];
#pragma unroll
            for (uint32_t x = 0; x < 4u; ++x) r += (j + x < end && o[x] < k) ? 1u : 0u;
        }
        keys[start + r] = ((d + 1u) << 12) | (4095u - k);
    }
    __syncthreads();
    return true;
}

constexpr int SORT_KEYS = 8192;

__global__ void __launch_bounds__(1024) k_rowsort(const ProbDesc* __restrict__ probs, ProbState* __restrict__ st,
                                                  BatchTotals* __restrict__ tot,
                                                  const uint32_t* __restrict__ rowCnt,
                                                  uint32_t* __restrict__ rowPos, uint32_t* __restrict__ perm,
                                                  uint32_t* __restrict__ sliceWidth, uint32_t* __restrict__ sliceBase,
                                                  uint32_t* __restrict__ listOff, long long capList, int skip0 /* stream-layout problems take k_lists */,
                                                  int eqMax /* place_keys(): rows of one degree at most; 0: always the bitonic sort */)
{
    // (static LDS of this kernel: ~70 KB — hist 32 KB, place_keys()' tables 24 KB, rows and degrees 12 KB.  gfx950 has 160 KB per
    //  workgroup; the 64 KB parts before it are NOT a target of this library: see the static_assert below and the Makefile)
    static_assert(sizeof(uint32_t) * (SORT_KEYS + 2 * STREAM_MAXL) + sizeof(uint16_t) * 2 * STREAM_MAXL <= 160 * 1024, "k_rowsort's tables must fit the LDS of a gfx950 workgroup");
    __shared__ uint32_t hist[SORT_KEYS];         // indexed by SORT_KEYS-1-key: ascending index = descending count
    __shared__ uint32_t wsum[20];
    __shared__ uint32_t hcntS[STREAM_MAXL], hcurS[STREAM_MAXL];     // place_keys(): rows per degree, cursor / end of the degree's range
    __shared__ uint16_t tmpS[STREAM_MAXL], dgS[STREAM_MAXL];        // ... the rows in their ranges (any order), the degrees
    __shared__ uint32_t carry_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nt = blockDim.x, nw = nt >> 6;
    const int L = st[b].L;
    const int64_t lo = probs[b].liveOff;
    if (st[b].kind >= 2) return;
    if (st[b].kind == 0 && skip0) return;
    if (st[b].kind == 0) {
        // stream layout: bitonic sort (descending) of the UNIQUE keys ((degree + 1) << 12) | (4095 - row): larger degree
        // first, equal degrees in row order — the rank is the row's position.  N = next power of two >= L keys in LDS
        // (padding keys 0 sort last), log2(N)(log2(N)+1)/2 <= 78 compare-exchange stages of N/2 pairs.
        static_assert(STREAM_MAXL <= 4096 && SORT_KEYS >= 4096, "bitonic sort capacity");
        int N = 64; while (N < L) N <<= 1;
        for (int t = tid; t < L; t += nt) dgS[t] = (uint16_t)rowCnt[lo + t];
        __syncthreads();
        // (round 5: the sorted key array without the sort — place_keys() above; the sort remains for live sets in which very many rows share a degree)
        if (eqMax <= 0 || !place_keys(L, N, eqMax, [&](int k) { return (uint32_t)dgS[k]; }, hist, hcntS, hcurS, tmpS, wsum)) {
        for (int t = tid; t < N; t += nt) hist[t] = (t < L) ? ((((uint32_t)dgS[t] + 1u) << 12) | (uint32_t)(4095 - t)) : 0u;
        __syncthreads();
        for (int k2 = 2; k2 <= N; k2 <<= 1)
            for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                for (int t = tid; t < (N >> 1); t += nt) {
                    const int i1 = ((t & ~(j2 - 1)) << 1) | (t & (j2 - 1)), i2 = i1 | j2;     // the pair (i1, i1 ^ j2)
                    const uint32_t a = hist[i1], c2 = hist[i2];
                    const bool desc = (i1 & k2) == 0;                                         // direction of this bitonic block
                    if ((a < c2) == desc) { hist[i1] = c2; hist[i2] = a; }
                }
                __syncthreads();
            }
        }
        for (int q = tid; q < L; q += nt) {
            const uint32_t k = 4095u - (hist[q] & 4095u);
            perm[lo + q] = k; rowPos[lo + k] = (uint32_t)q;
        }
        // Candidate lists (k_upper writes them, k_fill_list reads them): position q keeps at most
        // min(degree, L - 1 - q) of its candidates — room for that many 16-bit column indices, rounded up to whole
        // quads, at listOff[q] behind the problem's base.  The base comes from a bump pointer shared by the batch (where
        // a problem's lists lie is immaterial); a problem whose lists would end beyond the pool becomes kind 2.
        {
            const int PER = (L + nt - 1) / nt;                  // consecutive positions per thread (<= 3)
            uint32_t sum = 0;
            for (int t = 0; t < PER; ++t) {
                const int q = tid * PER + t;
                if (q < L) sum += (min((hist[q] >> 12) - 1u, (uint32_t)(L - 1 - q)) + 3u) & ~3u;
            }
            const uint32_t inc = wave_incl_scan(sum);
            if (lane == WAVE - 1) wsum[w] = inc;
            __syncthreads();
            uint32_t wbase = 0, total = 0;
            for (int t = 0; t < nw; ++t) { if (t < w) wbase += wsum[t]; total += wsum[t]; }
            if (tid == 0) {
                const unsigned long long base = atomicAdd(&tot->listTop, (unsigned long long)total);
                st[b].listOff = (int64_t)base;
                if ((long long)(base + total) > capList) { st[b].kind = 2; atomicAdd(&tot->overflow, 1); }
            }
            uint32_t run = wbase + inc - sum;
            for (int t = 0; t < PER; ++t) {
                const int q = tid * PER + t;
                if (q < L) { listOff[lo + q] = run; run += (min((hist[q] >> 12) - 1u, (uint32_t)(L - 1 - q)) + 3u) & ~3u; }
            }
        }
        return;                                                 // slice geometry of the stream layout: k_slicegeom
    }
    for (int t = tid; t < SORT_KEYS; t += nt) hist[t] = 0;
    __syncthreads();
    for (int k = tid; k < L; k += nt) atomicAdd(&hist[SORT_KEYS - 1 - min(rowCnt[lo + k], (uint32_t)(SORT_KEYS - 1))], 1u);
    __syncthreads();
    {   // exclusive scan of hist (8 consecutive bins per thread)
        constexpr int PER = SORT_KEYS / 1024;
        uint32_t loc[PER]; uint32_t sum = 0;
        for (int t = 0; t < PER; ++t) { loc[t] = hist[tid * PER + t]; sum += loc[t]; }
        const uint32_t inc = wave_incl_scan(sum);
        if (lane == WAVE - 1) wsum[w] = inc;
        __syncthreads();
        uint32_t wbase = 0;
        for (int t = 0; t < w; ++t) wbase += wsum[t];
        uint32_t run = wbase + inc - sum;
        for (int t = 0; t < PER; ++t) { hist[tid * PER + t] = run; run += loc[t]; }
    }
    __syncthreads();
    for (int k = tid; k < L; k += nt) {
        const uint32_t pos = atomicAdd(&hist[SORT_KEYS - 1 - min(rowCnt[lo + k], (uint32_t)(SORT_KEYS - 1))], 1u);
        rowPos[lo + k] = pos; perm[lo + pos] = (uint32_t)k;
    }
    __syncthreads();       // block-scope: perm visible to the whole workgroup
    const int nsl = (L + 63) >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int s0 = 0; s0 < nsl; s0 += nt) {
        const int s = s0 + tid;
        uint32_t width = 0;
        if (s < nsl) {
            const int hi = min(L, (s << 6) + 64);
            for (int p = s << 6; p < hi; ++p) width = max(width, rowCnt[lo + perm[lo + p]]);
            width = (width + 3u) & ~3u;                         // quad layout: 4 entries per lane and step
            sliceWidth[lo + s] = width;
        }
        const uint32_t v = width * 64u;
        const uint32_t inc = wave_incl_scan(v);
        if (lane == WAVE - 1) wsum[w] = inc;
        __syncthreads();
        uint32_t wbase = 0, tot = 0;
        for (int t = 0; t < nw; ++t) { if (t < w) wbase += wsum[t]; tot += wsum[t]; }
        const uint32_t carry = carry_s;
        if (s < nsl) sliceBase[lo + s] = carry + wbase + inc - v;
        __syncthreads();
        if (tid == 0) carry_s = carry + tot;
        __syncthreads();
    }
    if (tid == 0) st[b].nnzCap = carry_s;
}

// ---------------------------------------------------------------------------------------------
// k_upper (kind 0): which candidates row p of the stored matrix keeps.  The matrix is stored once per unordered pair:
// candidate (k, q) of the symmetric bit matrix stays in the row of the endpoint with the SMALLER position.  Row p of the
// result is row k = perm[p] of the live-order matrix with the bits q dropped whose position is not larger than p —
// the COLUMNS stay in live order (the fill kernel labels an entry with its column's position; the order of the entries
// inside a row is immaterial: the solver's sums are exact).  One wave per row: the row's words sit in its lanes (lane =
// word); for word w the lanes compare the positions of columns 64w..64w+63 (LDS table) with p, the ballot is ANDed
// onto the word (consecutive rows update the masks instead of rebuilding them).  The per-word prefix counts (entry index of a word's first kept candidate in k_fill_slice), the
// row's upper degree and the position-ordered copies of the pools the solver reads come out of the same pass.
// ---------------------------------------------------------------------------------------------
struct LivePools { int32_t* lp; int32_t* li; int32_t* lj; double* ls; double* ld; double* lza; double* lzb; };

__global__ void __launch_bounds__(1024) k_upper(const ProbDesc* __restrict__ probs, const ProbState* __restrict__ st,
                                                const BatchTotals* __restrict__ tot, const ItemDesc* __restrict__ items,
                                                const unsigned long long* __restrict__ maskPool,
                                                uint16_t* __restrict__ listPool, const uint32_t* __restrict__ listOff,
                                                uint32_t* __restrict__ rowCnt, const uint32_t* __restrict__ perm,
                                                const uint32_t* __restrict__ rowPos, LivePools src, LivePools dst, int RPB)
{
    __shared__ uint16_t posS[STREAM_MAXL + 64];                  // position of every live column (padding: 0 = never kept)
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6, wpb = nt >> 6;
    const int nItems = tot->items;
    int staged = -1;
    // XCD-aware order (workgroup ids are dealt to the 8 XCDs round-robin): XCD x takes the CONTIGUOUS range [x Gx, (x + 1) Gx) of
    // work items — the items of a problem, which share its tables, columns and mask rows, run on one L2
    const int Gx_ = (nItems + 7) >> 3;
    for (int sIdx_ = blockIdx.x; (sIdx_ >> 3) < Gx_; sIdx_ += gridDim.x) {
        const int t = (sIdx_ & 7) * Gx_ + (sIdx_ >> 3);
        if (t >= nItems) continue;
        const ItemDesc it = items[t];
        const int b = it.b;
        if (uni_i(st[b].kind) == 0) {                           // (no `continue` around the barriers below)
        const int L = st[b].L;
        const int W = (L + 63) >> 6;
        const int64_t lo = probs[b].liveOff, mo = st[b].maskOff;
        uint16_t* const lists = listPool + st[b].listOff;
        const int nrows = min(RPB, L - it.row0);
        if (staged != b) {                                       // consecutive items of a workgroup often share the problem
            __syncthreads();
            for (int q = tid; q < W * 64; q += nt) posS[q] = (q < L) ? (uint16_t)rowPos[lo + q] : (uint16_t)0;
            __syncthreads();
            staged = b;
        }
        // A wave takes CONSECUTIVE rows: the set of columns behind p loses exactly one member, column perm[p + 1], when p
        // moves on by one — the "behind" masks of all words are built once (lane = word) and then only updated.
        const int RW = (nrows + wpb - 1) / wpb;
        const int r0 = w * RW, r1 = min(nrows, r0 + RW);
        if (r0 < r1) {
            const int p0 = it.row0 + r0;
            uint32_t glo = 0u, ghi = 0u;                         // lane wd: columns of word wd with a position > p
            for (int wd = 0; wd < W; ++wd) {
                const unsigned long long gt = __ballot((int)posS[(wd << 6) + lane] > p0);
                writelane2(glo, ghi, gt, (uint32_t)__builtin_amdgcn_readfirstlane(wd));
            }
            unsigned long long behind = ((unsigned long long)ghi << 32) | glo;
            // the wave's rows: live index and list offset of row r0 + l in lane l (read back with v_readlane), and the
            // position-ordered copies of the pools the solver reads; the mask row of the NEXT row is requested before
            // the current one is worked on, so no memory round trip sits between two rows
            const int nr = r1 - r0;                              // <= RPB / waves per block <= 64
            const int kv = (lane < nr) ? (int)perm[lo + p0 + lane] : 0;
            const uint32_t ov = (lane < nr) ? listOff[lo + p0 + lane] : 0u;
            if (lane < nr) { dst.lp[lo + p0 + lane] = src.lp[lo + kv]; dst.ld[lo + p0 + lane] = src.ld[lo + kv]; }
            unsigned long long m_n = (lane < W) ? maskPool[mo + (int64_t)__builtin_amdgcn_readlane(kv, 0) * W + lane] : 0ull;
            for (int i = 0; i < nr; ++i) {
                const int p = p0 + i;                            // position of the row being written
                const unsigned long long raw = m_n;
                int kn = 0;
                if (i + 1 < nr) {
                    kn = __builtin_amdgcn_readlane(kv, i + 1);
                    m_n = (lane < W) ? maskPool[mo + (int64_t)kn * W + lane] : 0ull;
                }
                const unsigned long long mine = raw & behind;
                const uint32_t c = (uint32_t)__popcll(mine);
                const uint32_t ex = wave_excl_scan(c, lane);
                const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane((int)(ex + c), WAVE - 1);
                {   // the row's candidate list: live column indices in ascending order, padded to a whole quad
                    uint16_t* lst = lists + (uint32_t)__builtin_amdgcn_readlane((int)ov, i);
                    unsigned long long m = mine; uint32_t e = ex;
                    while (m) { lst[e++] = (uint16_t)((lane << 6) + __builtin_ctzll(m)); m &= m - 1ull; }
                    if (lane < 4 && cnt + (uint32_t)lane < ((cnt + 3u) & ~3u)) lst[cnt + lane] = (uint16_t)0xffffu;
                }
                if (lane == 0) rowCnt[lo + p] = cnt;             // upper degree of position p (the live-order degrees are spent)
                if (i + 1 < nr && lane == (kn >> 6)) behind &= ~(1ull << (kn & 63));   // the column at position p + 1 is no longer behind
            }
        }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_lists (kind 0; launches in which no fallback problem can occur): from the UPPER blocks of the candidate bit matrix — what
// k_count writes — straight to positions and kept-candidate lists, one workgroup per problem, everything that is looked up by
// index in LDS.  It stands for k_mirror + k_rowprefix + k_rowsort + k_upper, which reach the same lists through the symmetric
// matrix (0.55 MB per problem written and read again, four dependent launches: 0.31 ms of a 2.0 ms step at config 3):
//   degrees    a stored bit (k, q), k < q, counts for row k (popcount of the row's words) and for row q (one LDS atomic per
//              set bit): the full degree of the symmetric matrix without ever forming it;
//   positions  rank by (degree descending, row ascending): k_rowsort's bitonic sort of unique keys, in LDS;
//   lists      room for position p as k_rowsort sizes it (min(degree, L - 1 - p) entries, whole quads, bump pointer of the
//              batch); a second sweep over the bits hands every pair to its endpoint of SMALLER position (slot by an LDS
//              cursor, the other endpoint's live column index as the entry), then the rows are padded to whole quads and their
//              upper degrees written in position order with the position-ordered copies of the pools the solver reads.
// The ENTRIES of a list arrive in the order the cursors were taken, not ascending: where an entry sits in its row is immaterial
// (the fill labels it with its column's position, the solver's sums are exact integers) — roman_get_upper_csr sorts its rows.
// Sweep: 16 lanes per row, four rows per wave step, lane = one 64-column word of the row's upper part (the diagonal word keeps
// its bits behind the row's own); a row's words come in one or two coalesced 128-byte pieces.  In the second sweep the bit loop
// only queues the pairs (per-wave LDS queue); they are placed 256 at a time with every lane busy.  The lists are laid out in
// position order, so the problem's first winCap list entries are one range of the pool: they are built in dynamic LDS and
// written out in whole quads (512 contiguous bytes per wave store) instead of one 2-byte store each.
// ---------------------------------------------------------------------------------------------
constexpr int LISTS_NT = 1024;
constexpr int LISTS_QRUN = 256;           // pairs a wave places at once (four per lane)
constexpr int LISTS_QCAP = 512;           // queue entries per wave: a step's pairs go in at once when they fit (else 64 at a time)

__global__ void __launch_bounds__(LISTS_NT) k_lists(int B, const ProbDesc* __restrict__ probs, ProbState* __restrict__ st, BatchTotals* __restrict__ tot,
                                                   const unsigned long long* __restrict__ maskPool,
                                                   uint16_t* __restrict__ listPool, uint32_t* __restrict__ listOff,
                                                   uint32_t* __restrict__ rowCnt, uint32_t* __restrict__ perm, uint32_t* __restrict__ rowPos,
                                                   LivePools src, LivePools dst, long long capList,
                                                   int eqMax /* place_keys(): rows of one degree at most; 0: always the bitonic sort */,
                                                   int degGiven /* rowCnt holds every live row's full degree (k_count counted the pairs as they passed: whole problems): no degree sweep */,
                                                   int winCap /* list entries of the window in dynamic LDS (a multiple of 4; 0: every entry stored where it goes) */)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t winS[];    // the problem's first winCap list entries, written out in whole quads
    __shared__ uint32_t degS[STREAM_MAXL + 64];                 // full degree of a live row; after the sort: the row's list cursor
    __shared__ uint32_t keyS[(LISTS_NT / 64) * LISTS_QCAP];    // sort keys (4096); in the pair sweep: per wave, pairs (k << 16 | q) waiting to be placed
    __shared__ unsigned long long tabS[STREAM_MAXL + 64];       // per live row: list offset << 16 | position (one LDS read serves both); before: place_keys()' two tables
    __shared__ uint16_t tmpS[STREAM_MAXL + 64];                 // place_keys(): the rows in their degree's range; after: the row at position p
    __shared__ uint32_t wsum[LISTS_NT / 64 + 4];
    __shared__ int okS;
    static_assert(STREAM_MAXL <= 4096, "sort capacity");
    static_assert(LISTS_QRUN % 64 == 0 && LISTS_QCAP >= LISTS_QRUN + 64 && (LISTS_NT / 64) * LISTS_QCAP >= 4096, "k_lists queue");
    uint32_t* const qS = keyS;                                  // (the keys are spent once the lists have their room: the tail reads tmpS)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NW = LISTS_NT / 64;
    const int g = lane >> 4, sl = lane & 15;                    // row of the wave step, word of the row's piece
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();                                        // (the previous problem's LDS is no longer read)
        if (st[b].kind != 0) continue;
        const int L = st[b].L;
        if (L <= 0) continue;
        const int W = (L + 63) >> 6;
        const int64_t lo = probs[b].liveOff, mo = st[b].maskOff;
        const unsigned long long* mrow = maskPool + mo;
        // f(k, m, c): word c (strictly-upper bits only) of live row k, for every row and every word at or behind its diagonal one.
        // A wave step = four rows (one 64-row block: k0 is a multiple of four) x sixteen words from c0 on; the words of the next
        // six steps are in flight while one is worked on (unconditional loads at clamped addresses: the wait counters stay exact)
        auto fetch = [&](int k0_, int c0_) -> unsigned long long {
            const int k = k0_ + g, c = c0_ + sl;
            const bool valid = k < L && c < W;                  // (c >= k >> 6 by construction: c0 starts at the rows' diagonal word)
            unsigned long long m = mrow[(int64_t)min(k, L - 1) * W + min(c, W - 1)];
            if (!valid) m = 0ull;
            if (c == (k >> 6)) m &= ((k & 63) == 63) ? 0ull : (~0ull << ((k & 63) + 1));   // the diagonal block holds both triangles: columns behind k only
            return m;
        };
        auto advance = [&](int& k0_, int& c0_) { c0_ += 16; if (c0_ >= W) { k0_ += 4 * NW; c0_ = k0_ >> 6; } };
        auto sweep = [&](auto f) {
            constexpr int PF = 6;                               // steps in flight: a wave walks ~50 steps, each a dependent round trip otherwise
            int kr[PF], cr[PF]; unsigned long long mr[PF];
            int kn = 4 * w, cn = kn >> 6;
#pragma unroll
            for (int i = 0; i < PF; ++i) { kr[i] = kn; cr[i] = cn; mr[i] = fetch(kn, cn); advance(kn, cn); }
            while (kr[0] < L) {                                 // (steps are in ascending row order; a step behind the last row carries no bits)
#pragma unroll
                for (int i = 0; i < PF; ++i) {
                    const int kc = kr[i], cc = cr[i]; const unsigned long long mc = mr[i];
                    kr[i] = kn; cr[i] = cn; mr[i] = fetch(kn, cn); advance(kn, cn);
                    f(kc + g, mc, cc + sl);
                }
            }
        };
#ifdef ROMAN_LISTS_TIMING
        unsigned long long tl_[6]; tl_[0] = __builtin_readcyclecounter();
#define LMARK(i_) tl_[i_] = __builtin_readcyclecounter()
#else
#define LMARK(i_) do { } while (0)
#endif
        for (int q = tid; q < L; q += LISTS_NT) degS[q] = degGiven ? rowCnt[lo + q] : 0u;
        __syncthreads();
        // ---- degrees ----
        if (!degGiven) {
        sweep([&](int k, unsigned long long m, int c) {
            if (m) {
                atomicAdd(&degS[k], (uint32_t)__popcll(m));
                while (m) { atomicAdd(&degS[(c << 6) + __builtin_ctzll(m)], 1u); m &= m - 1ull; }
            }
        });
        __syncthreads();
        }
        LMARK(1);
        // ---- positions: bitonic sort (descending) of the unique keys ((degree + 1) << 12) | (4095 - row) (k_rowsort's order) ----
        int N = 64; while (N < L) N <<= 1;
        // (the sorted key array without the sort: place_keys(); its two tables of L words each lie in tabS, which is written behind this phase)
        if (eqMax <= 0 || !place_keys(L, N, eqMax, [&](int k) { return degS[k]; }, keyS, reinterpret_cast<uint32_t*>(tabS), reinterpret_cast<uint32_t*>(tabS) + (STREAM_MAXL + 64), tmpS, wsum)) {
        for (int t = tid; t < N; t += LISTS_NT) keyS[t] = (t < L) ? (((degS[t] + 1u) << 12) | (uint32_t)(4095 - t)) : 0u;
        __syncthreads();
        for (int k2 = 2; k2 <= N; k2 <<= 1)
            for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                for (int t = tid; t < (N >> 1); t += LISTS_NT) {
                    const int i1 = ((t & ~(j2 - 1)) << 1) | (t & (j2 - 1)), i2 = i1 | j2;
                    const uint32_t a = keyS[i1], c2 = keyS[i2];
                    const bool desc = (i1 & k2) == 0;
                    if ((a < c2) == desc) { keyS[i1] = c2; keyS[i2] = a; }
                }
                __syncthreads();                                // (stages inside a wave's own 128 keys without the barrier: measured, no faster)
            }
        }
        LMARK(2);
        // ---- list room per position (whole quads), the problem's base from the batch's bump pointer ----
        uint32_t total = 0;                                     // list entries of the problem (whole quads)
        {
            const int PER = (L + LISTS_NT - 1) / LISTS_NT;      // consecutive positions per thread (<= 3)
            uint32_t sum = 0;
            for (int t = 0; t < PER; ++t) {
                const int q = tid * PER + t;
                if (q < L) sum += (min((keyS[q] >> 12) - 1u, (uint32_t)(L - 1 - q)) + 3u) & ~3u;
            }
            const uint32_t inc = wave_incl_scan(sum);
            if (lane == WAVE - 1) wsum[w] = inc;
            __syncthreads();
            uint32_t wbase = 0;
            for (int t = 0; t < NW; ++t) { if (t < w) wbase += wsum[t]; total += wsum[t]; }
            if (tid == 0) {
                const unsigned long long base = atomicAdd(&tot->listTop, (unsigned long long)total);
                st[b].listOff = (int64_t)base;
                const bool fits = (long long)(base + total) <= capList;
                if (!fits) { st[b].kind = 2; atomicAdd(&tot->overflow, 1); }
                okS = fits ? 1 : 0;
            }
            uint32_t run = wbase + inc - sum;
            for (int t = 0; t < PER; ++t) {
                const int q = tid * PER + t;
                if (q < L) {
                    const uint32_t k = 4095u - (keyS[q] & 4095u);
                    perm[lo + q] = k; rowPos[lo + k] = (uint32_t)q; tmpS[q] = (uint16_t)k;
                    tabS[k] = ((unsigned long long)run << 16) | (unsigned long long)q; listOff[lo + q] = run; degS[k] = 0u;     // (degS: now the row's list cursor)
                    run += (min((keyS[q] >> 12) - 1u, (uint32_t)(L - 1 - q)) + 3u) & ~3u;
                }
            }
        }
        __syncthreads();
        if (!okS) continue;                                     // lists beyond the pool: skipped like any workspace overflow (the history now knows the need)
        uint16_t* const lists = listPool + st[b].listOff;
        LMARK(3);
        // ---- every stored pair to its endpoint of smaller position ----
        // The sweep's per-lane bit loop only appends (k << 16 | q) to the wave's queue (offsets from a scan of the words'
        // popcounts); the pairs are placed LISTS_QRUN at a time with every lane busy (a word has 1.8 set bits on average, a wave
        // step runs to its lanes' maximum, ~6.5: 28 % of the lanes placed pairs inside the bit loop)
        {
        uint32_t* const qw = qS + w * LISTS_QCAP;
        uint32_t qn = 0;                                        // queue fill (wave-uniform)
        auto lds_order = [&]() {                                // LDS operations of one wave execute in order: this is for the compiler
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        // four pairs per lane: every LDS read of the four requested before the first is used, then the four cursor atomics
        auto place = [&](uint32_t base, uint32_t n, auto full) {
            constexpr int CH = LISTS_QRUN / WAVE;
            uint32_t kk[CH], qq[CH], slot[CH]; unsigned long long tk[CH], tq[CH]; bool act[CH];
#pragma unroll
            for (int x = 0; x < CH; ++x) {
                const uint32_t idx = (uint32_t)(x * WAVE + lane);
                act[x] = decltype(full)::value || idx < n;
                const uint32_t e = qw[base + (act[x] ? idx : 0u)];
                kk[x] = e >> 16; qq[x] = e & 0xffffu;
                tk[x] = tabS[kk[x]]; tq[x] = tabS[qq[x]];
            }
#pragma unroll
            for (int x = 0; x < CH; ++x) {
                const bool mine = ((uint32_t)tk[x] & 0xffffu) < ((uint32_t)tq[x] & 0xffffu);   // the pair belongs to its endpoint of smaller position
                if (act[x]) slot[x] = atomicAdd(&degS[mine ? kk[x] : qq[x]], 1u);
            }
#pragma unroll
            for (int x = 0; x < CH; ++x) {
                const bool mine = ((uint32_t)tk[x] & 0xffffu) < ((uint32_t)tq[x] & 0xffffu);
                const uint32_t at = (uint32_t)((mine ? tk[x] : tq[x]) >> 16) + slot[x];
                const uint16_t v = (uint16_t)(mine ? qq[x] : kk[x]);
                if (act[x]) { if (at < (uint32_t)winCap) winS[at] = v; else lists[at] = v; }
            }
        };
        auto drain = [&]() {
            if (qn >= (uint32_t)LISTS_QRUN) {
                lds_order();
                while (qn >= (uint32_t)LISTS_QRUN) { qn -= LISTS_QRUN; place(qn, LISTS_QRUN, std::true_type{}); }
                lds_order();
            }
        };
        sweep([&](int k, unsigned long long m, int c) {
            const uint32_t cnt = (uint32_t)__popcll(m);
            const uint32_t incl = wave_incl_scan(cnt);
            const uint32_t npairs = (uint32_t)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
            const uint32_t kq = ((uint32_t)k << 16) | (uint32_t)(c << 6);
            if (qn + npairs <= (uint32_t)LISTS_QCAP) {
                uint32_t at = qn + incl - cnt;
                while (m) { qw[at++] = kq + (uint32_t)__builtin_ctzll(m); m &= m - 1ull; }
                qn += npairs;
            } else {
                // a step with more pairs than the queue has room for (dense rows): 64 at a time, placed in between
                while (true) {
                    const unsigned long long bm = __ballot(m != 0ull);
                    if (bm == 0ull) break;
                    if (m) {
                        qw[qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u))] = kq + (uint32_t)__builtin_ctzll(m);
                        m &= m - 1ull;
                    }
                    qn += (uint32_t)__popcll(bm);
                    drain();
                }
            }
            drain();
        });
        lds_order();
        if (qn) place(0u, qn, std::false_type{});
        }
        __syncthreads();
        LMARK(4);
        // ---- padding, upper degrees and the position-ordered pools ----
        for (int p = tid; p < L; p += LISTS_NT) {
            const uint32_t k = tmpS[p];
            const uint32_t cnt = degS[k];
            rowCnt[lo + p] = cnt;
            const uint32_t o = (uint32_t)(tabS[k] >> 16);
            for (uint32_t e = o + cnt; e < o + ((cnt + 3u) & ~3u); ++e) { if (e < (uint32_t)winCap) winS[e] = (uint16_t)0xffffu; else lists[e] = (uint16_t)0xffffu; }
            dst.lp[lo + p] = src.lp[lo + k]; dst.ld[lo + p] = src.ld[lo + k];
        }
        {   // the window: whole quads (8 bytes: a problem's lists start at a multiple of four entries), 512 contiguous bytes per wave store
            const uint32_t nq = min(total, (uint32_t)winCap) >> 2;
            __syncthreads();
            for (uint32_t i = (uint32_t)tid; i < nq; i += LISTS_NT)
                reinterpret_cast<uint2*>(lists)[i] = reinterpret_cast<const uint2*>(winS)[i];
        }
#ifdef ROMAN_LISTS_TIMING
        LMARK(5);
        if (tid == 0 && (b & 63) == 0) printf("[k_lists] b=%d L=%d cycles: degrees %llu sort %llu offsets %llu scatter %llu tail %llu\n", b, L,
                                              tl_[1] - tl_[0], tl_[2] - tl_[1], tl_[3] - tl_[2], tl_[4] - tl_[3], tl_[5] - tl_[4]);
#endif
#undef LMARK
    }
}

// k_slicegeom (kind 0): slice widths (longest upper row of the slice, rounded up to whole quads), slice bases and the
// problem's slot total.  One wave per problem, lane = slice.
__global__ void __launch_bounds__(64) k_slicegeom(const ProbDesc* __restrict__ probs, ProbState* __restrict__ st,
                                                  const uint32_t* __restrict__ rowCnt,
                                                  uint32_t* __restrict__ sliceWidth, uint32_t* __restrict__ sliceBase)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (st[b].kind != 0) return;
    const int L = st[b].L;
    const int64_t lo = probs[b].liveOff;
    const int nsl = (L + 63) >> 6;                                // <= STREAM_MAXL / 64 <= 64
    uint32_t width = 0;
    if (lane < nsl) {
        const int hi = min(L, (lane << 6) + 64);
        for (int p = lane << 6; p < hi; ++p) width = max(width, rowCnt[lo + p]);
        width = (width + 3u) & ~3u;
        sliceWidth[lo + lane] = width;
    }
    const uint32_t v = width * 64u;
    const uint32_t ex = wave_excl_scan(v, lane);
    if (lane < nsl) sliceBase[lo + lane] = ex;
    if (lane == WAVE - 1) st[b].nnzCap = ex + v;
}

// k_probscan: prefix over the problems of the per-problem slot totals and of the slice-group counts (k_fill_slice work items:
// min(NG, slices) groups of consecutive slices per stream-layout problem).  A problem whose matrix segment would end beyond
// `capNnz` slots becomes kind 2 (skipped; nothing has been written for it yet).
__global__ void __launch_bounds__(1024) k_probscan(int B, int NG /* fill groups per problem */, long long capNnz, ProbState* __restrict__ st, BatchTotals* __restrict__ tot)
{
    // one workgroup, PER consecutive problems per thread (k_rowbase)
    __shared__ long long shl[17];
    __shared__ int shi[17];
    __shared__ int red[1];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int PER = (B + nt - 1) / nt;
    const int b0 = tid * PER, b1 = min(B, b0 + PER);
    constexpr int PC = 8;                                        // (k_rowbase: the thread's problems are read once)
    int cK[PC], cL[PC]; uint32_t cC[PC];
#pragma unroll
    for (int j = 0; j < PC; ++j) { const int b = b0 + j; const bool in = j < PER && b < b1; cK[j] = in ? st[b].kind : 2; cL[j] = in ? st[b].L : 0; cC[j] = in ? st[b].nnzCap : 0u; }
    auto get = [&](int b, int& kind, int& L, long long& cap) {
        const int j = b - b0;
        if (j < PC) {
#pragma unroll
            for (int t = 0; t < PC; ++t) if (t == j) { kind = cK[t]; L = cL[t]; cap = (long long)cC[t]; }
        } else { kind = st[b].kind; L = st[b].L; cap = (long long)st[b].nnzCap; }
        if (kind >= 2) cap = 0;
    };
    long long sC = 0;
    for (int b = b0; b < b1; ++b) { int kind, L; long long cap; get(b, kind, L, cap); sC += cap; }
    long long totC; int totG;
    const long long baseC = block_excl_scan(sC, shl, totC);
    int sG = 0;
    {
        long long acc = baseC;
        for (int b = b0; b < b1; ++b) {
            int kind, L; long long cap; get(b, kind, L, cap);
            acc += cap;
            if (kind == 0 && acc <= capNnz) sG += min(NG, (L + 63) >> 6);
        }
    }
    const int baseG = block_excl_scan(sG, shi, totG);
    if (tid == 0) red[0] = 0;
    __syncthreads();
    int nover = 0;
    {
        long long acc = baseC; int gacc = baseG;
        for (int b = b0; b < b1; ++b) {
            int kind, L; long long cap; get(b, kind, L, cap);
            const bool fits = acc + cap <= capNnz;
            const int ng = (kind == 0 && fits) ? min(NG, (L + 63) >> 6) : 0;
            st[b].nnzOff = fits ? acc : 0; st[b].sgBase = gacc;
            if (!fits && kind < 2) { st[b].kind = 2; ++nover; }
            acc += cap; gacc += ng;
        }
    }
    for (int off = 32; off > 0; off >>= 1) nover += __shfl_xor(nover, off);
    if ((tid & 63) == 0 && nover) atomicAdd(&red[0], nover);
    __syncthreads();
    if (tid == 0) { tot->nnzTotal = totC < capNnz ? totC : capNnz; tot->sliceGroups = totG; tot->needNnz = totC; tot->overflow += red[0]; }
}

// ---------------------------------------------------------------------------------------------
// k_fill: candidates -> values, as ONE flat stream over the mask words of a work item (RPB rows x
// ceil(L/64) words, contiguous in HBM).  Each lane takes a mask word together with the candidate
// count in front of it; in every "bit step" each lane that still has set bits emits one candidate
// (row, column, entry index) into the wave's LDS ring.  Whenever 64 candidates are queued the wave
// evaluates them densely, whatever rows they belong to: x (recomputed bit-identically from the
// tables), sqrt/exp/cbrt, fusion with the two single scores, the affinityeps filter, and the store
// into the row's SELL slot column.  The problem's per-association data (objects, z, single score,
// SELL slot base) is staged in LDS once per work item.  Finally every row's slot column is padded
// to the slice width with inert entries.
// ---------------------------------------------------------------------------------------------
constexpr int FILL_E = 1;            // candidates a lane evaluates at a time (2: measured without gain, 212 B of scratch)
constexpr int FILL_Q = 256;          // ring capacity per wave (>= 64 FILL_E queued + 64 emitted per bit step)

// The rows of a k_fill work item (at most FILL_RPB consecutive positions) in LDS: live row, objects, single score, z, slice base + lane slot
constexpr int FILL_RPB = 128;
struct FillRows { int32_t* k; int32_t* i; int32_t* j; uint32_t* base; double* s; double* za; double* zb; };
constexpr int FILL_ROWBYTES = 4 * 4 + 3 * 8;    // per row

// CM: where an entry's per-association data comes from — 1: the problem's whole column tile in LDS (rows and columns); 2: a WINDOW of
// columns [wq0, wq0 + 64 Ww) in LDS, the item's rows from their own small tile (FillRows)
template <bool GRAV, typename IdxT, int CM, bool QUAD>
__device__ __forceinline__ uint32_t fill_item(const DevParams& D, const ProbDesc& pd, int L, int row0, int nrows, int wq0, int Ww,
                                              int w, int wpb, int lane,
                                              const int32_t* cI, const int32_t* cJ, const double* cS,
                                              const double* cZa, const double* cZb, const uint32_t* cBase, const uint32_t* cPos,
                                              const double* __restrict__ TA, const double* __restrict__ TB,
                                              const unsigned long long* __restrict__ mbase, const uint32_t* __restrict__ pbase,
                                              const FillRows& R /* the item's rows (R.k: position row0 + r -> live row: an item is a block of consecutive POSITIONS) */,
                                              uint32_t* qK, uint32_t* qQ, uint32_t* qE,
                                              IdxT* __restrict__ cols, double* __restrict__ vals)
{
    constexpr bool LDSCOL = CM == 1;
    const int W = (L + 63) >> 6;
    const int64_t nwords = (int64_t)nrows * Ww;
    const int w0 = wq0 >> 6;
    // The item's rows are the rows at positions row0 .. row0 + nrows - 1: what it writes is a few consecutive slices of the matrix (a
    // 128-byte line of the quad layout holds 16 bytes of each of eight NEIGHBOURING positions — with items of consecutive live rows its
    // eight parts arrived from eight workgroups at eight different times: eight partial writes per line)
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t head = 0, queued = 0, upper = 0;

    // up to FILL_E x 64 queued candidates at a time, FILL_E per lane: their record reads, then their table reads, are in flight together
    // (one candidate per lane was a chain of two dependent L2 round trips per 64 entries and wave: the kernel was bound by that latency,
    //  not by its gathers' number — packing seven arrays into one record changed nothing, 6.0 ms per 64 x L = 10 000 either way)
    auto evaluate = [&](uint32_t take) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        bool on[FILL_E]; int rl[FILL_E], k[FILL_E], q[FILL_E]; uint32_t e[FILL_E];
        int i[FILL_E], j[FILL_E], iq[FILL_E], jq[FILL_E]; double sk[FILL_E], sq[FILL_E], dz[FILL_E];
        uint32_t base[FILL_E], pk[FILL_E], pq[FILL_E];       // slice base + lane slot (base is a multiple of 64); positions of row and column
#pragma unroll
        for (int h = 0; h < FILL_E; ++h) {
            const uint32_t idx = (uint32_t)lane + 64u * (uint32_t)h;
            on[h] = idx < take;
            const uint32_t s = (head + (on[h] ? idx : 0u)) & (FILL_Q - 1);    // (an idle lane repeats the first candidate's reads; it stores nothing)
            rl[h] = (int)qK[s]; k[h] = R.k[rl[h]]; q[h] = (int)qQ[s]; e[h] = qE[s];
        }
#pragma unroll
        for (int h = 0; h < FILL_E; ++h) {
            if (LDSCOL) {
                i[h] = cI[k[h]]; j[h] = cJ[k[h]]; iq[h] = cI[q[h]]; jq[h] = cJ[q[h]]; sk[h] = cS[k[h]]; sq[h] = cS[q[h]];
                dz[h] = GRAV ? (cZa[k[h]] - cZa[q[h]]) - (cZb[k[h]] - cZb[q[h]]) : 0.0;
                base[h] = cBase[k[h]]; pk[h] = cPos[k[h]]; pq[h] = cPos[q[h]];
            } else {
                const int r_ = rl[h], ql = q[h] - wq0;
                i[h] = R.i[r_]; j[h] = R.j[r_]; iq[h] = cI[ql]; jq[h] = cJ[ql]; sk[h] = R.s[r_]; sq[h] = cS[ql];
                dz[h] = GRAV ? (R.za[r_] - cZa[ql]) - (R.zb[r_] - cZb[ql]) : 0.0;
                base[h] = R.base[r_]; pk[h] = (uint32_t)(row0 + r_); pq[h] = cPos[ql];
            }
        }
        double a[FILL_E], bb[FILL_E];
#pragma unroll
        for (int h = 0; h < FILL_E; ++h) { a[h] = TA[(int64_t)i[h] * pd.n1 + iq[h]]; bb[h] = TB[(int64_t)j[h] * pd.n2 + jq[h]]; }
#pragma unroll
        for (int h = 0; h < FILL_E; ++h) {
            double c;
            if (GRAV && D.gmode != 3) {
                const double ch = fabs(a[h] - bb[h]);
                const double hm = a[h] > bb[h] ? a[h] : bb[h];
                double cv = fabs(dz[h]) - D.sin_unc * hm;
                if (cv < 0.0) cv = 0.0;
                c = sqrt(ch * ch + cv * cv);
            } else {
                c = fabs(a[h] - bb[h]);                         // no gravity prior, or the z-gate reading (full lengths)
            }
            const double sa = fx_exp(((-0.5 * c) * c) / D.sig2);
            const double v = fuse_pair(D, sa, sk[h], sq[h]);
            const bool keep = v > D.p.affinityeps;
            // an entry at or below affinityeps belongs neither to M nor to C: inert slot
            // column labels are POSITIONS (sorted row order): the solvers keep their vectors in that order
            if (on[h]) {
                cols[col_pos<QUAD>(base[h] & ~63u, base[h] & 63u, e[h])] = keep ? (IdxT)pq[h] : fb_inert<IdxT>(pk[h]);
                vals[val_pos<QUAD>(base[h] & ~63u, base[h] & 63u, e[h])] = keep ? v : 0.0;
                upper += (keep && q[h] > k[h]) ? 1u : 0u;
            }
        }
        head = (head + take) & (FILL_Q - 1); queued -= take;
    };

    const int64_t nblk = (nwords + 63) >> 6;
    unsigned long long m_next = 0ull; uint32_t p_next = 0u, k_next = 0u;
    auto fetch = [&](int64_t x_) {                              // word x_ of the item's flat stream: live row, mask word, entries in front of it
        const int r_ = (int)x_ / Ww;                            // (RPB * W < 2^31)
        const int64_t a_ = (int64_t)R.k[r_] * W + (w0 + ((int)x_ - r_ * Ww));
        k_next = (uint32_t)r_; m_next = mbase[a_]; p_next = pbase[a_];
    };
    {   // prefetch the wave's first block
        const int64_t x = (int64_t)w * 64 + lane;
        if (w < nblk && x < nwords) fetch(x);
    }
    for (int64_t blk = w; blk < nblk; blk += wpb) {
        unsigned long long m = m_next; uint32_t e = p_next; const uint32_t kl = k_next;     // (kl: the word's row of the item)
        const int64_t x = blk * 64 + lane;
        {   // prefetch the next block while this one is expanded / evaluated
            const int64_t xn = x + (int64_t)wpb * 64;
            m_next = 0ull; p_next = 0u;
            if (blk + wpb < nblk && xn < nwords) fetch(xn);
        }
        const uint32_t qb = (uint32_t)(w0 + ((int)x - ((int)x / Ww) * Ww)) << 6;  // first column of this word
        for (;;) {                                              // bit steps
            const bool has = m != 0ull;
            const unsigned long long act = __ballot(has);
            if (act == 0ull) break;
            if (has) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1ull;
                const uint32_t s = (head + queued + (uint32_t)__popcll(act & lt)) & (FILL_Q - 1);
                qK[s] = kl; qQ[s] = qb + (uint32_t)bit; qE[s] = e;
                ++e;
            }
            queued += (uint32_t)__popcll(act);
            while (queued >= 64u * FILL_E) evaluate(64u * FILL_E);
        }
    }
    while (queued > 0u) evaluate(min(queued, 64u * (uint32_t)FILL_E));
    return upper;
}

template <bool GRAV, typename IdxT, bool QUAD>
__global__ void __launch_bounds__(1024) k_fill(DevParams D, const ProbDesc* __restrict__ probs,
                                               ProbState* __restrict__ st,
                                               const BatchTotals* __restrict__ tot,
                                               const ItemDesc* __restrict__ items,
                                               const double* __restrict__ tabPool,
                                               const int32_t* __restrict__ li, const int32_t* __restrict__ lj,
                                               const double* __restrict__ ls,
                                               const double* __restrict__ lza, const double* __restrict__ lzb,
                                               const uint32_t* __restrict__ rowCnt,
                                               const unsigned long long* __restrict__ maskPool,
                                               const uint32_t* __restrict__ prefPool,
                                               const uint32_t* __restrict__ rowPos,
                                               const uint32_t* __restrict__ sliceWidth,
                                               const uint32_t* __restrict__ sliceBase,
                                               IdxT* __restrict__ cols, double* __restrict__ vals, int TC, int RPB /* <= FILL_RPB */,
                                               const uint32_t* __restrict__ permPool /* position -> live row */)
{
    // LDS: cS[TC] [GRAV: cZa[TC] cZb[TC]] cI[TC] cJ[TC] cBase[TC] cPos[TC] | per-wave rings qK qQ qE
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* cS = reinterpret_cast<double*>(smem);
    double* cZa = cS + TC;
    double* cZb = cZa + (GRAV ? TC : 0);
    int32_t* cI = reinterpret_cast<int32_t*>(cZb + (GRAV ? TC : 0));
    int32_t* cJ = cI + TC;
    uint32_t* cBase = reinterpret_cast<uint32_t*>(cJ + TC);
    uint32_t* cPos = cBase + TC;
    uint32_t* rings = cPos + TC;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, w = tid >> 6, wpb = nt >> 6;
    FillRows R;                                                  // behind the rings: the item's rows
    R.s = reinterpret_cast<double*>(rings + (size_t)wpb * 3 * FILL_Q); R.za = R.s + FILL_RPB; R.zb = R.za + FILL_RPB;
    R.k = reinterpret_cast<int32_t*>(R.zb + FILL_RPB); R.i = R.k + FILL_RPB; R.j = R.i + FILL_RPB; R.base = reinterpret_cast<uint32_t*>(R.j + FILL_RPB);
    uint32_t* qK = rings + (size_t)w * 3 * FILL_Q;
    uint32_t* qQ = qK + FILL_Q;
    uint32_t* qE = qQ + FILL_Q;
    const int nItems = tot->items;
    // XCD-aware order (workgroup ids are dealt to the 8 XCDs round-robin): XCD x takes the CONTIGUOUS range [x Gx, (x + 1) Gx) of
    // work items — the items of a problem, which share its tables, columns and mask rows, run on one L2
    // A workgroup takes a UNIT of FILL_RPB / RPB consecutive items and fills the runs of items of one problem in it as ONE item of up to
    // FILL_RPB rows: what an item stages — a window of columns per ~2 800 live associations — does not depend on its rows (64 x L = 10 000:
    // 6.0 / 3.9 / 2.8 ms with items of 32 / 64 / 128 rows; the other kernels of the build keep the item size that suits them)
    const int gpu_ = max(1, FILL_RPB / RPB);
    const int nUnits = (nItems + gpu_ - 1) / gpu_;
    const int Gx_ = (nUnits + 7) >> 3;
    for (int sIdx_ = blockIdx.x; (sIdx_ >> 3) < Gx_; sIdx_ += gridDim.x) {
        const int u_ = (sIdx_ & 7) * Gx_ + (sIdx_ >> 3);
        if (u_ >= nUnits) continue;
        const int tEnd_ = min(nItems, (u_ + 1) * gpu_);
        for (int t = u_ * gpu_; t < tEnd_; ) {
        ItemDesc it = items[t];
        const int b = it.b;
        int te_ = t + 1;
        while (te_ < tEnd_ && items[te_].b == b) ++te_;         // (the items of a problem follow each other, in row order)
        const int nIt_ = te_ - t;
        t = te_;
        if (uni_i(st[b].kind) == 1) {           // stream-layout problems are filled by k_fill_slice, skipped ones not at all
        const ProbDesc pd = probs[b];
        const int L = st[b].L;
        const int64_t lo = pd.liveOff, mo = st[b].maskOff, no = st[b].nnzOff;
        const int nrows = min(nIt_ * RPB, L - it.row0);
        const double* TA = tabPool + pd.tabOff;
        const double* TB = TA + (int64_t)pd.n1 * pd.n1;
        const bool ldscol = L <= TC;
        __syncthreads();                        // every wave is done with the previous item's columns and rows
        for (int r = tid; r < nrows; r += nt) {
            const uint32_t pos = (uint32_t)(it.row0 + r);
            const int k = (int)permPool[lo + pos];
            R.k[r] = k; R.i[r] = li[lo + k]; R.j[r] = lj[lo + k]; R.s[r] = ls[lo + k];
            if (GRAV) { R.za[r] = lza[lo + k]; R.zb[r] = lzb[lo + k]; }
            R.base[r] = sliceBase[lo + (pos >> 6)] + (pos & 63u);
        }
        if (ldscol) {
            for (int q = tid; q < L; q += nt) {
                cI[q] = li[lo + q]; cJ[q] = lj[lo + q]; cS[q] = ls[lo + q];
                if (GRAV) { cZa[q] = lza[lo + q]; cZb[q] = lzb[lo + q]; }
                const uint32_t pos = rowPos[lo + q];
                cBase[q] = sliceBase[lo + (pos >> 6)] + (pos & 63u); cPos[q] = pos;
            }
        }
        __syncthreads();
        uint32_t upper = 0u;
        if (ldscol)
            upper = fill_item<GRAV, IdxT, 1, QUAD>(D, pd, L, it.row0, nrows, 0, (L + 63) >> 6, w, wpb, lane, cI, cJ, cS, cZa, cZb, cBase, cPos, TA, TB,
                                                maskPool + mo, prefPool + mo, R, qK, qQ, qE, cols + no, vals + no);
        else {
            // live sets beyond the tile: WINDOWS of TC columns (a multiple of 64), one after the other — the window's columns into LDS
            // (coalesced), the item's word stream restricted to the window's words; an entry then costs its two table reads and its two
            // stores instead of fifteen requests to the L2
            const int TCw = TC & ~63;
            for (int q0 = 0; q0 < L; q0 += TCw) {
                const int qn = min(TCw, L - q0);
                if (q0 > 0) __syncthreads();    // every wave is done with the previous window's columns
                for (int q = tid; q < qn; q += nt) {
                    const int64_t g_ = lo + q0 + q;
                    cI[q] = li[g_]; cJ[q] = lj[g_]; cS[q] = ls[g_];
                    if (GRAV) { cZa[q] = lza[g_]; cZb[q] = lzb[g_]; }
                    cPos[q] = rowPos[g_];
                }
                __syncthreads();
                upper += fill_item<GRAV, IdxT, 2, QUAD>(D, pd, L, it.row0, nrows, q0, (qn + 63) >> 6, w, wpb, lane, cI, cJ, cS, cZa, cZb, cBase, cPos, TA, TB,
                                                        maskPool + mo, prefPool + mo, R, qK, qQ, qE, cols + no, vals + no);
            }
        }
        // pad every row's slot column up to its slice width with inert entries (value 0, C-flag; the
        // column is the row's own position: a real, finite vector element whatever the solver gathers from)
        for (int r = w; r < nrows; r += wpb) {
            const uint32_t pos = (uint32_t)(it.row0 + r);        // (items are blocks of positions)
            const int k = (int)permPool[lo + pos];
            const uint32_t width = sliceWidth[lo + (pos >> 6)];
            const int64_t sb = no + sliceBase[lo + (pos >> 6)];
            for (uint32_t e = rowCnt[lo + k] + lane; e < width; e += WAVE) {
                cols[col_pos<QUAD>(sb, pos & 63u, e)] = fb_inert<IdxT>(pos);
                vals[val_pos<QUAD>(sb, pos & 63u, e)] = 0.0;
            }
        }
        if (QUAD && it.row0 + nrows == L && (L & 63)) {         // lane slots of the last slice that hold no row
            const uint32_t sl = (uint32_t)(L >> 6);
            const uint32_t width = sliceWidth[lo + sl];
            const int64_t sb = no + sliceBase[lo + sl];
            const uint32_t nfree = 64u - (uint32_t)(L & 63);
            for (uint32_t x = tid; x < nfree * width; x += nt) {
                const uint32_t slot = (uint32_t)(L & 63) + x / width, e = x % width;
                cols[col_pos<QUAD>(sb, slot, e)] = fb_inert<IdxT>(0u);                   // (column 0, flagged: gathers a real element, adds nothing)
                vals[val_pos<QUAD>(sb, slot, e)] = 0.0;
            }
        }
        for (int off = 32; off > 0; off >>= 1) upper += __shfl_xor(upper, off);
        if (lane == 0 && upper) atomicAdd(&st[b].nnzUpper, (unsigned long long)upper);
        }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_fill_list (stream layout): candidates -> values, written straight into the quad layout.  k_upper left every
// position row's kept candidates as a list of live column indices (ascending, padded to whole quads), so entry e of a
// row is simply element e of its list.  A slice is 64 rows x (longest list, in quads) SLOT quads; a row's list covers
// only its first slot quads, and at the workload's shapes a third of the (slot quad, row) pairs have no list quad.
// Only the pairs that have one are evaluated.  Per window of FILL_WIN consecutive slot quads of a work item:
//   pass 1  lane = row, slot quads dealt to the waves: ballot of the rows whose list reaches the slot quad -> mask, count
//           and slice of the slot quad in LDS; the other lanes write their slot inert (slice padding: value 0, the lane
//           slot's dummy column with the C-flag);
//   scan    one wave: live pairs in front of every slot quad;
//   pass 2  the live pairs in (slot quad, row) order, 64 consecutive ones per wave step: a lane finds its slot quad in the
//           prefix table (the wave's first one by bisection, its own by stepping on) and its row as the n-th set bit of
//           the mask, then: one 8-byte list read, four independent evaluation chains (two LDS column lookups, two table
//           gathers, sqrt / exp / cbrt, fusion, affinityeps filter), one 8-byte column store and two 16-byte value
//           stores — the layout's own order, contiguous over the wave wherever the live rows of a slot quad are.
// Entries beyond a row's count in its last quad and filtered entries are written inert by pass 2.  Every slot is written
// exactly once, with what the lane = row loop wrote there.  Work items are groups of consecutive slices of one problem (NG
// groups per problem): the problem's column tile (objects, z, single score, position of every live association) is staged
// in LDS once per item, as are the rows of the group (live index, count, list offset).  Items are ordered so that the
// groups of one problem run on one XCD (its tables stay in that L2).
// ---------------------------------------------------------------------------------------------
constexpr int FILLS_MAXSPI = STREAM_MAXL / 64;     // slices per work item (group): up to a whole problem

template <bool GRAV, bool FAST>
__device__ __forceinline__ double fill_value(const DevParams& D, double a, double bb, double dza, double dzb, double ss, double sk, double sq)
{
    double c;
    if (GRAV && D.gmode != 3) {
        const double ch = fabs(a - bb);
        const double hm = a > bb ? a : bb;
        double cv = fabs(dza - dzb) - D.sin_unc * hm;
        if (cv < 0.0) cv = 0.0;
        c = sqrt(ch * ch + cv * cv);
    } else {
        c = fabs(a - bb);                   // no gravity prior, or the z-gate reading (full lengths)
    }
    const double sa = fx_exp(((-0.5 * c) * c) / D.sig2);
    if (FAST) return (sa == 0.0) ? 0.0 : fx_cbrt(sa * ss);      // geometric mean, distance weight 1: fuse_pair()'s default branch
    return fuse_pair(D, sa, sk, sq);
}

constexpr uint32_t FILL_ROTATE = 5;      // k_fill_list rotates the list quads of row x by FILL_ROTATE * x (why: at the rotation itself)
constexpr int FILL_WIN = 256;            // slot quads of a group k_fill_list takes between two barriers (its mask / prefix tables in LDS)

// Index of the n-th set bit (n = 0: the lowest) of the 64-bit mask hi:lo; n < popcount.
__device__ __forceinline__ uint32_t nth_set_bit(uint32_t lo, uint32_t hi, uint32_t n)
{
    uint32_t base = 0, v = lo;
    const uint32_t c = (uint32_t)__popc(lo);
    if (n >= c) { n -= c; v = hi; base = 32; }
#pragma unroll
    for (int s = 16; s > 0; s >>= 1) {
        const uint32_t cl = (uint32_t)__popc(v & ((1u << s) - 1u));
        if (n >= cl) { n -= cl; v >>= s; base += (uint32_t)s; }
    }
    return base;
}

template <bool GRAV, bool FAST, bool OBJ>
__global__ void __launch_bounds__(1024) k_fill_list(DevParams D, int B, const ProbDesc* __restrict__ probs,
                                                    ProbState* __restrict__ st, const BatchTotals* __restrict__ tot,
                                                    const double* __restrict__ tabPool, const double* __restrict__ feats, int NO /* OBJ: object capacity per map */,
                                                    const int32_t* __restrict__ li, const int32_t* __restrict__ lj,
                                                    const double* __restrict__ ls,
                                                    const double* __restrict__ lza, const double* __restrict__ lzb,
                                                    const uint16_t* __restrict__ listPool, const uint32_t* __restrict__ listOff,
                                                    const uint32_t* __restrict__ rowCnt,
                                                    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ rowPos,
                                                    const uint32_t* __restrict__ sliceWidth,
                                                    const uint32_t* __restrict__ sliceBase,
                                                    uint16_t* __restrict__ cols, double* __restrict__ vals, int TC, int NG, int SPI /* LDS capacity: slices per group */)
{
    // LDS: cS[TC] [OBJ: sO[2*NO] (x, y, z, -) | else GRAV: cZa[TC] cZb[TC]] cI[TC] cJ[TC] | gK gCnt gOff [SPI*64] | gQ[SPI+1] gSB[SPI+1] | wLo wHi wSl [FILL_WIN] wPre[FILL_WIN+1] | cP[TC] (u16)
    // OBJ: the two distances of an entry are RECOMPUTED from the objects' coordinates (LDS) with k_tables' own operation
    // sequence — the same bits — instead of gathered from the tables: a wave's 64 lanes are 64 different rows, every table
    // gather touched 64 cache lines for 64 doubles (4 GB of L2 -> L1 line traffic per batch of 256 at config 3, the kernel's bound).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* cS = reinterpret_cast<double*>(smem);
    dbl2_t* sO = reinterpret_cast<dbl2_t*>(cS + TC);            // object o of map 1: sO[2o], sO[2o+1]; of map 2: sO[2(NO+o)], ...
    double* cZa = OBJ ? cS + TC + 8 * NO : cS + TC;
    double* cZb = cZa + ((GRAV && !OBJ) ? TC : 0);
    int32_t* cI = reinterpret_cast<int32_t*>(cZb + ((GRAV && !OBJ) ? TC : 0));
    int32_t* cJ = cI + TC;
    uint32_t* gK = reinterpret_cast<uint32_t*>(cJ + TC);         // rows of the group's slices: live index (~0: no row)
    uint32_t* gCnt = gK + SPI * 64;                     //   kept candidates
    uint32_t* gOff = gCnt + SPI * 64;                   //   list offset
    uint32_t* gQ = gOff + SPI * 64;                     // quads in front of every slice of the group (+ total)
    uint32_t* gSB = gQ + SPI + 1;                       // slice bases
    uint32_t* wLo = gSB + SPI + 1;                      // window: live-row mask of every slot quad (low, high half)
    uint32_t* wHi = wLo + FILL_WIN;
    uint32_t* wSl = wHi + FILL_WIN;                     //   its slice inside the group
    uint32_t* wPre = wSl + FILL_WIN;                    //   live quads in front of it (+ the total, at [FILL_WIN])
    uint16_t* cP = reinterpret_cast<uint16_t*>(wPre + FILL_WIN + 1);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, w = tid >> 6, nw = nt >> 6;
    const int nGroups = tot->sliceGroups;
    // XCD-aware order: workgroups are dealt to the 8 XCDs round-robin by id, so XCD x takes the CONTIGUOUS range
    // [x*Gx, (x+1)*Gx) of groups — the groups of one problem (which share its tables) run on one L2.
    const int Gx = (nGroups + 7) >> 3;
    for (int sIdx = blockIdx.x; (sIdx >> 3) < Gx; sIdx += gridDim.x) {
        const int t = (sIdx & 7) * Gx + (sIdx >> 3);
        if (t < nGroups) {
        int b = 0;                                              // last problem with sgBase <= t and at least one group
        {
            int lo_ = 0, hi_ = B - 1;
            while (lo_ < hi_) { const int mid = (lo_ + hi_ + 1) >> 1; if (st[mid].sgBase <= t) lo_ = mid; else hi_ = mid - 1; }
            b = lo_;
        }
        const ProbDesc pd = probs[b];
        const int L = st[b].L;
        const int W = (L + 63) >> 6;
        const int64_t lo = pd.liveOff, no = st[b].nnzOff;
        const uint16_t* lists = listPool + st[b].listOff;
        // every problem is cut into the same number of groups (min(NG, W)) of ceil(W / groups) slices: with a uniform
        // batch the static deal then hands every workgroup the same mix of heavy (first) and light (last) groups
        const int ngb = min(NG, W), spib = (W + ngb - 1) / max(ngb, 1);
        const int s_begin = (t - st[b].sgBase) * spib, s_end = min(W, s_begin + spib), ns = max(s_end - s_begin, 0);
        const double* TA = tabPool + pd.tabOff;
        const double* TB = TA + (int64_t)pd.n1 * pd.n1;
        __syncthreads();                        // every wave is done with the previous group's tile
        for (int q = tid; q < L; q += nt) {
            cI[q] = li[lo + q]; cJ[q] = lj[lo + q]; cS[q] = ls[lo + q]; cP[q] = (uint16_t)rowPos[lo + q];
            if (GRAV && !OBJ) { cZa[q] = lza[lo + q]; cZb[q] = lzb[lo + q]; }
        }
        if (OBJ) {
            const int pdim = D.p.point_dim;
            for (int o = tid; o < pd.n1 + pd.n2; o += nt) {
                const double* f = feats + (o < pd.n1 ? pd.off1 + o : pd.off2 + (o - pd.n1)) * D.F;
                const int slot = o < pd.n1 ? o : NO + (o - pd.n1);
                sO[2 * slot] = dbl2_t{f[0], pdim > 1 ? f[1] : 0.0};
                sO[2 * slot + 1] = dbl2_t{pdim > 2 ? f[2] : 0.0, 0.0};
            }
        }
        const bool horiz = D.gmode == 1 || D.gmode == 2;        // the tables hold horizontal distances (k_tables)
        for (int x = tid; x < ns * 64; x += nt) {
            const int p = s_begin * 64 + x;
            const bool row = p < L;
            gK[x] = row ? perm[lo + p] : 0xffffffffu; gCnt[x] = row ? rowCnt[lo + p] : 0u; gOff[x] = row ? listOff[lo + p] : 0u;
        }
        if (w == 0) {                           // quads in front of every slice of the group
            const uint32_t wq = (lane < ns) ? (sliceWidth[lo + s_begin + lane] >> 2) : 0u;
            const uint32_t ex = wave_excl_scan(wq, lane);
            if (lane < ns) { gQ[lane] = ex; gSB[lane] = sliceBase[lo + s_begin + lane]; }
            if (lane == ns) gQ[ns] = ex;        // ns <= STREAM_MAXL / 64 < 64
        }
        __syncthreads();
        const uint32_t Q = gQ[ns];
        uint32_t upper = 0;
        int si1 = 0;                                            // pass 1's slice (a wave's slot quads only go forward)
        for (uint32_t u0 = 0; u0 < Q; u0 += (uint32_t)FILL_WIN) {
            const uint32_t Wn = min((uint32_t)FILL_WIN, Q - u0);
            if (u0) __syncthreads();                            // every wave is done with the previous window's tables
            // Pass 1, lane = row, the window's slot quads dealt to the waves: which rows have a list quad for slot quad u
            // (mask, count); the others' slots are written inert here (slice padding: value 0, the lane slot's dummy column).
            for (uint32_t ul = (uint32_t)w; ul < Wn; ul += (uint32_t)nw) {
                const uint32_t u = u0 + ul;
                while (u >= gQ[si1 + 1]) ++si1;                 // wave-uniform
                const uint32_t g = u - gQ[si1];
                const bool live = g < ((gCnt[si1 * 64 + lane] + 3u) >> 2);
                const unsigned long long m = __ballot(live);
                if (lane == 0) { wLo[ul] = (uint32_t)m; wHi[ul] = (uint32_t)(m >> 32); wSl[ul] = (uint32_t)si1; wPre[ul] = (uint32_t)__popcll(m); }
                if (!live) {
                    const int64_t sb = no + gSB[si1];
                    const uint32_t inert = ((uint32_t)L + (uint32_t)lane) | 0x8000u, i2 = inert | (inert << 16);
                    *reinterpret_cast<uint2*>(cols + sb + (int64_t)g * 256 + lane * 4) = make_uint2(i2, i2);
                    *reinterpret_cast<double2*>(vals + sb + (int64_t)(2 * g) * 128 + lane * 2) = make_double2(0.0, 0.0);
                    *reinterpret_cast<double2*>(vals + sb + (int64_t)(2 * g + 1) * 128 + lane * 2) = make_double2(0.0, 0.0);
                }
            }
            for (uint32_t ul = Wn + (uint32_t)tid; ul < (uint32_t)FILL_WIN; ul += (uint32_t)nt) wPre[ul] = 0u;
            __syncthreads();
            if (w == 0) {                       // counts -> live quads in front of every slot quad, the window's total behind them
                static_assert(FILL_WIN == 4 * WAVE, "one wave scans the window, four slot quads per lane");
                uint32_t c[4], s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = wPre[4 * lane + j]; s += c[j]; }
                uint32_t ex = wave_excl_scan(s, lane);
#pragma unroll
                for (int j = 0; j < 4; ++j) { wPre[4 * lane + j] = ex; ex += c[j]; }
                if (lane == WAVE - 1) wPre[FILL_WIN] = ex;
            }
            __syncthreads();
            // Pass 2: the window's live (slot quad, row) pairs, in that order, 64 consecutive ones per wave step.
            const uint32_t F = wPre[FILL_WIN];
            for (uint32_t f0 = (uint32_t)uni_i(w) * 64u; f0 < F; f0 += (uint32_t)nt) {
            uint32_t ul = 0;                                    // wave-uniform: the slot quad of the wave's first pair
            { uint32_t lo_ = 0, hi_ = Wn - 1u; while (lo_ < hi_) { const uint32_t mid = (lo_ + hi_ + 1u) >> 1; if (wPre[mid] <= f0) lo_ = mid; else hi_ = mid - 1u; } ul = lo_; }
            const uint32_t f = f0 + (uint32_t)lane;
            if (f < F) {
            while (wPre[ul + 1] <= f) ++ul;                     // (every slot quad of a slice has a live row: at most 64 steps; wPre[Wn] = F > f)
            const int r = (int)nth_set_bit(wLo[ul], wHi[ul], f - wPre[ul]);       // the pair's row: lane slot r of its slice
            const int si = (int)wSl[ul];
            const uint32_t g = u0 + ul - gQ[si];
            const int64_t sb = no + gSB[si];                    // first element of the slice (multiple of 256)
            const int x = si * 64 + r;
            const uint32_t kraw = gK[x], cnt = gCnt[x];
            // Which list quad goes into slot quad g: the row's quads ROTATED by a row-dependent offset.  The order of a row's
            // entries is free (the solver's sums are exact), and the 64 rows of a slice — lanes of one wave — hold much the same
            // columns in the same (live-index) order: unrotated, the lanes of a solver step push onto the same few columns at
            // once (LDS atomics onto one address serialise: SQ_LDS_BANK_CONFLICT 0.55 of the LDS-active cycles of k_solve_up).
            // Measured (round 4, two boxes, alternating): solver launch in flight 1.41-1.45 -> 1.36-1.37 ms, p50 0.665-0.674 -> 0.640 ms,
            // throughput +0.5-1.5 %, isolated solver launch 1.09-1.11 -> 1.02-1.03 ms.  Starting lane l at l/64 of its row instead, with or
            // without a further rotation inside the quad: 1.04-1.06 ms, p50 0.64-0.65 (same boxes, alternating): the plain one stays.
            const uint32_t nq = (cnt + 3u) >> 2;                // > g: the pair is live
            const uint32_t e0 = ((g + (uint32_t)x * FILL_ROTATE) % nq) << 2;
            const uint2 qq = *reinterpret_cast<const uint2*>(lists + gOff[x] + e0);
            const int k = (int)kraw;
            const double sk = cS[k];
            const double* TAr = TA + (int64_t)cI[k] * pd.n1;
            const double* TBr = TB + (int64_t)cJ[k] * pd.n2;
            const double zak = (GRAV && !OBJ) ? cZa[k] : 0.0, zbk = (GRAV && !OBJ) ? cZb[k] : 0.0;
            dbl2_t oa0 = {0.0, 0.0}, oa1 = {0.0, 0.0}, ob0 = {0.0, 0.0}, ob1 = {0.0, 0.0};
            if (OBJ) { oa0 = sO[2 * cI[k]]; oa1 = sO[2 * cI[k] + 1]; ob0 = sO[2 * (NO + cJ[k])]; ob1 = sO[2 * (NO + cJ[k]) + 1]; }
            const uint32_t inert = ((uint32_t)L + (uint32_t)r) | 0x8000u;        // the lane slot's own dummy column
            uint32_t cw[4]; double vv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool have = e0 + (uint32_t)j < cnt;
                const uint32_t qr = ((j < 2 ? qq.x : qq.y) >> (16 * (j & 1))) & 0xffffu;
                const int q = have ? (int)qr : k;               // (a padding entry evaluates the row against itself: discarded)
                double a, bb, dza, dzb;
                if (OBJ) {                                      // k_tables' sequence: dx*dx + dy*dy (+ dz*dz), one correctly rounded sqrt
                    const dbl2_t pa0 = sO[2 * cI[q]], pa1 = sO[2 * cI[q] + 1], pb0 = sO[2 * (NO + cJ[q])], pb1 = sO[2 * (NO + cJ[q]) + 1];
                    const double dxa = oa0.x - pa0.x, dya = oa0.y - pa0.y, dxb = ob0.x - pb0.x, dyb = ob0.y - pb0.y;
                    dza = oa1.x - pa1.x; dzb = ob1.x - pb1.x;
                    const double h2a = dxa * dxa + dya * dya, h2b = dxb * dxb + dyb * dyb;
                    a = horiz ? sqrt(h2a) : sqrt(h2a + dza * dza);
                    bb = horiz ? sqrt(h2b) : sqrt(h2b + dzb * dzb);
                } else {
                    a = TAr[cI[q]]; bb = TBr[cJ[q]];
                    dza = GRAV ? zak - cZa[q] : 0.0; dzb = GRAV ? zbk - cZb[q] : 0.0;
                }
                if (!have) { a = 0.0; bb = 0.0; }
                const double sq = cS[q];
                const double v = fill_value<GRAV, FAST>(D, a, bb, GRAV ? dza : 0.0, GRAV ? dzb : 0.0, sk * sq, sk, sq);
                const bool keep = have && v > D.p.affinityeps;  // otherwise the slot stays inert: neither in M nor in C
                cw[j] = keep ? (uint32_t)cP[q] : inert;
                vv[j] = keep ? v : 0.0;
                upper += keep ? 1u : 0u;                        // every stored entry is kept once: a strict-upper one
            }
            *reinterpret_cast<uint2*>(cols + sb + (int64_t)g * 256 + r * 4) = make_uint2(cw[0] | (cw[1] << 16), cw[2] | (cw[3] << 16));
            *reinterpret_cast<double2*>(vals + sb + (int64_t)(2 * g) * 128 + r * 2) = make_double2(vv[0], vv[1]);
            *reinterpret_cast<double2*>(vals + sb + (int64_t)(2 * g + 1) * 128 + r * 2) = make_double2(vv[2], vv[3]);
            }
            }
        }
        for (int off = 32; off > 0; off >>= 1) upper += __shfl_xor(upper, off);
        if (lane == 0 && upper) atomicAdd(&st[b].nnzUpper, (unsigned long long)upper);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Dense problems (roman_set_matrix_data: the set_matrix_data / solve loop of [REF roman/align/object_registration.py:60-72]).
// The caller's M and C (n x n, row major) become the layouts the scored problems use, on the device: k_dense_mask writes
// the symmetric candidate bit matrix, the kernels of the scored path (k_rowprefix, k_rowsort, k_upper, k_slicegeom,
// k_probscan) turn it into positions, lists and slice geometry, k_dense_fill writes labels and values.  Like upstream
// only the STRICT UPPER triangles are read: entry (k, q) is M[min][max] / C[min][max]; it is stored when either is
// non-zero and carries the C flag when C is zero there.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void dense_entry(const double* __restrict__ M, const double* __restrict__ C, int n, int k, int q, double& mv, double& cv)
{
    const int a = min(k, q), b = max(k, q);
    mv = M[(int64_t)a * n + b]; cv = C[(int64_t)a * n + b];
}

__global__ void __launch_bounds__(256) k_dense_mask(int n, const double* __restrict__ M, const double* __restrict__ C,
                                                    unsigned long long* __restrict__ mask /* n rows x ceil(n/64) words */,
                                                    int* __restrict__ flags /* [0]: some stored entry has C == 0 */)
{
    const int lane = threadIdx.x & 63;
    const int W = (n + 63) >> 6;
    const int nwaves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int k = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); k < n; k += nwaves) {
        bool cz = false;
        for (int w = 0; w < W; ++w) {
            const int q = (w << 6) + lane;
            bool cand = false;
            if (q < n && q != k) {
                double mv, cv;
                dense_entry(M, C, n, k, q, mv, cv);
                cand = (mv != 0.0) || (cv != 0.0);
                cz = cz || (cand && cv == 0.0);
            }
            const unsigned long long m = __ballot(cand);
            if (lane == 0) mask[(int64_t)k * W + w] = m;
        }
        if (__ballot(cz) != 0ull && lane == 0) atomicOr(flags, 1);
    }
}

// flags[1] |= 1 when a weight of the strict upper triangle lies outside [0, 1] or is not finite: such a matrix must not take
// the stream solver, whose fixed-point sums assume 0 <= v <= 1 (host: roman_set_matrix_data).
__global__ void __launch_bounds__(256) k_dense_range(int n, const double* __restrict__ M, int* __restrict__ flags)
{
    const int lane = threadIdx.x & 63;
    const int nwaves = (int)(gridDim.x * (blockDim.x >> 6));
    bool bad = false;
    for (int k = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); k < n; k += nwaves)
        for (int q = k + 1 + lane; q < n; q += 64) {
            const double v = M[(int64_t)k * n + q];
            bad = bad || !(v >= 0.0 && v <= 1.0);               // (a NaN fails both comparisons)
        }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(flags + 1, 1);
}

// One thread per slot of the problem's matrix segment (slot t of the COLUMN array; the value sits at val_pos of the same
// (slice, lane slot, entry)).  KIND 0: stream layout — entry e of position row p is element e of its candidate list;
// padding points at the dummy element n + lane slot.  KIND 1: symmetric sorted SELL-64 in quads — entry e of row k is the
// e-th set bit of its mask row (per-word prefix counts from k_rowprefix); padding = the row's own position, flagged.
template <int KIND>
__global__ void __launch_bounds__(256) k_dense_fill(int n, const double* __restrict__ M, const double* __restrict__ C,
                                                    ProbState* __restrict__ st,
                                                    const uint32_t* __restrict__ rowCnt, const uint32_t* __restrict__ rowPos, const uint32_t* __restrict__ perm,
                                                    const uint32_t* __restrict__ sliceWidth, const uint32_t* __restrict__ sliceBase,
                                                    const uint16_t* __restrict__ listPool, const uint32_t* __restrict__ listOff,
                                                    const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ pref,
                                                    uint16_t* __restrict__ cols16, uint32_t* __restrict__ cols32, double* __restrict__ vals)
{
    const uint32_t total = st[0].nnzCap;
    const int64_t no = st[0].nnzOff;
    const int nsl = (n + 63) >> 6, W = nsl;
    const uint16_t* lists = listPool + st[0].listOff;
    unsigned upper = 0;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        int sl = 0;
        {   // last slice with sliceBase <= t (slices of width 0 share a base with their successor: skipped by the search)
            int lo_ = 0, hi_ = nsl - 1;
            while (lo_ < hi_) { const int mid = (lo_ + hi_ + 1) >> 1; if (sliceBase[mid] <= t) lo_ = mid; else hi_ = mid - 1; }
            sl = lo_;
        }
        const uint32_t sb = sliceBase[sl], off = t - sb;
        const uint32_t slot = (off & 255u) >> 2, e = ((off >> 8) << 2) | (off & 3u);
        const int pos = sl * 64 + (int)slot;
        const int k = pos < n ? (int)perm[pos] : -1;
        double val = 0.0;
        if (KIND == 0) {
            uint32_t label = ((uint32_t)n + slot) | 0x8000u;
            if (k >= 0 && e < rowCnt[pos]) {
                const int q = (int)lists[listOff[pos] + e];
                double mv, cv;
                dense_entry(M, C, n, k, q, mv, cv);
                label = rowPos[q] | (cv == 0.0 ? 0x8000u : 0u); val = mv; ++upper;
            }
            cols16[no + t] = (uint16_t)label;
        } else {
            uint32_t label = (uint32_t)(k >= 0 ? pos : 0) | 0x80000000u;
            if (k >= 0 && e < rowCnt[k]) {
                const unsigned long long* mrow = mask + (int64_t)k * W;
                const uint32_t* prow = pref + (int64_t)k * W;
                int lo_ = 0, hi_ = W - 1;                        // last word with prefix <= e
                while (lo_ < hi_) { const int mid = (lo_ + hi_ + 1) >> 1; if (prow[mid] <= e) lo_ = mid; else hi_ = mid - 1; }
                unsigned long long m = mrow[lo_];
                for (uint32_t i = prow[lo_]; i < e; ++i) m &= m - 1ull;
                const int q = (lo_ << 6) + __builtin_ctzll(m);
                double mv, cv;
                dense_entry(M, C, n, k, q, mv, cv);
                label = rowPos[q] | (cv == 0.0 ? 0x80000000u : 0u); val = mv;
                if (q > k) ++upper;
            }
            cols32[no + t] = label;
        }
        vals[no + val_pos<true>(sb, slot, e)] = val;
    }
    for (int off = 32; off > 0; off >>= 1) upper += __shfl_xor(upper, off);
    if ((threadIdx.x & 63) == 0 && upper) atomicAdd(&st[0].nnzUpper, (unsigned long long)upper);
}

// ---------------------------------------------------------------------------------------------
// solver
// ---------------------------------------------------------------------------------------------

struct SolveOut {           // device pointers of the batch outputs
    int32_t* assoc_out; int32_t* n_assoc_out; double* T_out; int32_t* status_out;
    roman_stats_t* stats_out; int32_t kmax;
    int32_t* nodesOrig;     // row pool: selected nodes as original association indices
    int32_t* nSel;          // per problem: number of selected nodes (untruncated)
    double*  uOut;          // row pool: final u over live associations
    unsigned long long* dbg;   // timing build only: 16 counters per problem
};

// Sum of (a, b) over the block, identical in every thread; fixed reduction tree.  `red` holds two
// ping-pong scratch areas of 32 doubles (`par` flips on every call), so consecutive reductions need a
// single barrier each: a buffer is rewritten only after the barrier of the following reduction.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red, int& par, int tid, int nw)
{
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    double* rr = red + 32 * par;
    par ^= 1;
    if ((tid & 63) == 0) { rr[2 * (tid >> 6)] = a; rr[2 * (tid >> 6) + 1] = b; }
    __syncthreads();
    double ra = 0.0, rb = 0.0;
    for (int i = 0; i < nw; ++i) { ra += rr[2 * i]; rb += rr[2 * i + 1]; }
    a = ra; b = rb;
}

// (M_off u)_p and (C_off u)_p for every position p from the fallback layout (symmetric sorted SELL-64 in quads: the 4 column
// words of entries 4g..4g+3 of a lane are one 16-byte load, the values two 16-byte loads): a wave owns a slice (lane = row
// slot) and walks the quads, G quads in flight.  Padding entries — and the lane slots of the last slice that hold no
// row — are inert (value 0, C-flag, a valid column), so there are no predicates.
typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));
template <typename IdxT, int G>
__device__ __forceinline__ void spmv_sell(const double* u, int L, const uint32_t* __restrict__ perm,
                                          const uint32_t* __restrict__ sliceWidth, const uint32_t* __restrict__ sliceBase,
                                          const IdxT* __restrict__ cols, const double* __restrict__ vals,
                                          double* Mu, double* Cu, int tid, int nt)
{
    static_assert(sizeof(IdxT) == 4, "fallback layout: 32-bit column words");
    const int lane = tid & 63, w = tid >> 6, nw = nt >> 6;
    const int nsl = (L + 63) >> 6;
    for (int s = w; s < nsl; s += nw) {
        const int pos = (s << 6) + lane;
        const bool valid = pos < L;
        const uint32_t nq = sliceWidth[s] >> 2;
        const uint4_t* cp = reinterpret_cast<const uint4_t*>(cols + sliceBase[s]) + lane;
        const dbl2_t* vp = reinterpret_cast<const dbl2_t*>(vals + sliceBase[s]) + lane;
        double am = 0.0, ac = 0.0;
        for (uint32_t g0 = 0; g0 < nq; g0 += G) {
            uint4_t c_[G]; dbl2_t v0_[G], v1_[G];
#pragma unroll
            for (int t = 0; t < G; ++t) {
                const uint32_t g = min(g0 + (uint32_t)t, nq - 1u);      // (clamped: a repeated quad is skipped below)
                c_[t] = cp[(size_t)g * 64]; v0_[t] = vp[(size_t)(2 * g) * 64]; v1_[t] = vp[(size_t)(2 * g + 1) * 64];
            }
#pragma unroll
            for (int t = 0; t < G; ++t) {
                if (g0 + (uint32_t)t < nq) {
                    const uint32_t c4[4] = {c_[t].x, c_[t].y, c_[t].z, c_[t].w};
                    const double v4[4] = {v0_[t].x, v0_[t].y, v1_[t].x, v1_[t].y};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double uq = u[c4[e] & IdxTraits<IdxT>::MASK];
                        am = fma(v4[e], uq, am);
                        ac += (c4[e] & IdxTraits<IdxT>::CZ) ? 0.0 : uq;
                    }
                }
            }
        }
        if (valid) { Mu[pos] = am; Cu[pos] = ac; }
    }
}

// One-sided Jacobi (Hestenes) SVD of a dxd matrix (d = 2 or 3), then the proper rotation
// R = u1 v1' + u2 v2' + (u1 x u2)(v1 x v2)'   — equal to the reference's  U Vh  with the last
// row of Vh negated when det = -1 ([REF roman/align/object_registration.py:121-126]).
__device__ __forceinline__ double wave_sum63(double v);       // (defined with the stream solver's reductions below)
__device__ __forceinline__ double readlane63(double v);

// One-sided Jacobi step on the column pair (P, Q) of G (V accumulates the rotations).  Everything is indexed at compile time:
// G and V stay in registers (the round-1 form walked p, q, r with run-time indices — 76 scratch accesses of ~500 cycles each
// on the one thread that runs it: 47 k cycles per alignment, a twentieth of a config-3 solve and half of a demo-scale one).
template <int P, int Q>
__device__ __forceinline__ void jacobi_pair(double (&G)[9], double (&V)[9], bool& moved)
{
    double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) { al += G[r * 3 + P] * G[r * 3 + P]; be += G[r * 3 + Q] * G[r * 3 + Q]; ga += G[r * 3 + P] * G[r * 3 + Q]; }
    if (ga == 0.0) return;
    const double ab = al * be, g2 = ga * ga;                    // |ga| <= 1e-17 sqrt(al be), squared (no square root on the one thread's critical path)
    if (g2 <= 1e-34 * ab) return;
    if (!(g2 < 1e-30 * ab)) moved = true;                      // the sweep still found a pair of columns that is not orthogonal to working precision
    // t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), zeta = (be - al) / (2 ga), with numerator and denominator multiplied by |2 ga|:
    // one division and one square root instead of two and one; c = 1 / sqrt(1 + t^2) as a reciprocal square root
    const double a2 = be - al, b2 = 2.0 * ga;
    const double t = (((a2 >= 0.0) == (b2 >= 0.0)) ? fabs(b2) : -fabs(b2)) / (fabs(a2) + sqrt(a2 * a2 + b2 * b2));
    const double c = rsqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double gp = G[r * 3 + P], gq = G[r * 3 + Q];
        G[r * 3 + P] = c * gp - s * gq; G[r * 3 + Q] = s * gp + c * gq;
        const double vp = V[r * 3 + P], vq = V[r * 3 + Q];
        V[r * 3 + P] = c * vp - s * vq; V[r * 3 + Q] = s * vp + c * vq;
    }
}
// column c (run-time index) of a 3 x 3 matrix held in registers
__device__ __forceinline__ double col3(const double (&A)[9], int r3, int c) { return c == 0 ? A[r3] : (c == 1 ? A[r3 + 1] : A[r3 + 2]); }

// Rotation of the Kabsch / Umeyama fit from the d x d cross-covariance H (d = 2 or 3; rows and columns >= d of H are ignored):
// one-sided Jacobi SVD of H, the two leading singular pairs, the third by cross products (a proper rotation whatever the rank).
// `thin` (optional, 8 doubles): where the 3-D fit found rank H <= 1 and completed u1 arbitrarily, thin[0] = 1, thin[1..6] = u1, v1
// and thin[7] = s1
// — a caller that still has the points can then settle the turn about the line (wave_pose).
__device__ __forceinline__ void kabsch_rotation(const double (&H)[9], int d, double (&R)[9], double* thin = nullptr)
{
    double G[9], V[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G[r * 3 + c] = (r < d && c < d) ? H[r * 3 + c] : 0.0;
            V[r * 3 + c] = (r == c) ? 1.0 : 0.0;
            R[r * 3 + c] = 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {                 // (d == 2: the pairs with column 2 find ga == 0 and return)
        bool moved = false;
        jacobi_pair<0, 1>(G, V, moved);
        jacobi_pair<0, 2>(G, V, moved);
        jacobi_pair<1, 2>(G, V, moved);
        if (!moved) break;
    }
    double sg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { double s = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) s += G[r * 3 + c] * G[r * 3 + c];
        sg[c] = sqrt(s); }
    int i1 = 0;
#pragma unroll
    for (int c = 1; c < 3; ++c) if (c < d && sg[c] > (i1 == 0 ? sg[0] : (i1 == 1 ? sg[1] : sg[2]))) i1 = c;
    int i2 = -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) if (c < d && c != i1 && (i2 < 0 || sg[c] > (i2 == 0 ? sg[0] : (i2 == 1 ? sg[1] : sg[2])))) i2 = c;
    const double s1 = i1 == 0 ? sg[0] : (i1 == 1 ? sg[1] : sg[2]), s2 = i2 == 0 ? sg[0] : (i2 == 1 ? sg[1] : sg[2]);
    double u1[3] = {0, 0, 0}, u2[3] = {0, 0, 0}, v1[3] = {0, 0, 0}, v2[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 3; ++r) if (r < d) { v1[r] = col3(V, r * 3, i1); v2[r] = col3(V, r * 3, i2); }
    if (s1 > 0.0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) if (r < d) u1[r] = col3(G, r * 3, i1) / s1;
    } else { u1[0] = 1.0; }                                             // H == 0: any rotation
    if (d == 2) {
        // R = u1 v1' + perp(u1) perp(v1)'
        const double pu[2] = {-u1[1], u1[0]}, pv[2] = {-v1[1], v1[0]};
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) R[r * 3 + c] = u1[r] * v1[c] + pu[r] * pv[c];
        return;
    }
    if (s2 > 1e-300 && s2 > 1e-14 * s1) {
#pragma unroll
        for (int r = 0; r < 3; ++r) u2[r] = col3(G, r * 3, i2) / s2;
    } else {                                                            // rank <= 1: complete u1 arbitrarily
        if (thin != nullptr && s1 > 0.0) {
            thin[0] = 1.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) { thin[1 + r] = u1[r]; thin[4 + r] = v1[r]; }
            thin[7] = s1;
        }
        int m = 0;
        if (fabs(u1[1]) < fabs(u1[0])) m = 1;
        if (fabs(u1[2]) < fabs(m == 0 ? u1[0] : u1[1])) m = 2;
        const double dp = m == 0 ? u1[0] : (m == 1 ? u1[1] : u1[2]);
        double nn = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) { u2[r] = (r == m ? 1.0 : 0.0) - dp * u1[r]; nn += u2[r] * u2[r]; }
        nn = sqrt(nn);
#pragma unroll
        for (int r = 0; r < 3; ++r) u2[r] /= nn;
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
}

// T (row-major (d+1)x(d+1) in the leading entries of 16 doubles) from centred sums.
__device__ __forceinline__ void store_pose(double (&T)[16], int d, const double (&R)[9], const double (&m1)[3], const double (&m2)[3])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) T[t] = 0.0;
    if (d == 3) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double tr = m1[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) { T[r * 4 + c] = R[r * 3 + c]; tr -= R[r * 3 + c] * m2[c]; }
            T[r * 4 + 3] = tr;
        }
        T[15] = 1.0;
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double tr = m1[r];
#pragma unroll
            for (int c = 0; c < 2; ++c) { T[r * 3 + c] = R[r * 3 + c]; tr -= R[r * 3 + c] * m2[c]; }
            T[r * 3 + 2] = tr;
        }
        T[8] = 1.0;
    }
}
__device__ __forceinline__ void write_pose(double (&T)[16], int d, const double (&H)[9], const double (&m1)[3], const double (&m2)[3],
                                           double* thin = nullptr)
{
    double R[9];
    kabsch_rotation(H, d, R, thin);
    store_pose(T, d, R, m1, m2);
}

// The turn about the line of a rank-1 fit.  H2 is the cross-covariance of the points with their u1 / v1 components taken out (a
// needle's cross-section: far below the rounding of H itself, s2 / s1 < 2^-53, yet held by the coordinates).  Its leading singular
// pair, made orthogonal to (u1, v1), replaces the arbitrary completion.  False — the completion stays — where that pair is no
// more than rounding: H2 of points on one line is noise of about 2^-104 s1 (the squared rounding of the deflated coordinates; 0.2 to
// 0.9 of it measured for lines inside +-15 of the origin), a needle of cross-section 1e-9 gives 1e13 times that; the line is drawn
// at 2^-90 s1.  (Far from the origin the centroids' rounding alone is (c / r)^2 larger and can pass the line: the turn is then set by
// that noise — as proper and as optimal as the completion.)
__device__ __forceinline__ bool thin_rotation(const double* thin, const double (&H2)[9], double (&R)[9])
{
    double G[9], V[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) { G[e] = H2[e]; V[e] = (e % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool moved = false;
        jacobi_pair<0, 1>(G, V, moved);
        jacobi_pair<0, 2>(G, V, moved);
        jacobi_pair<1, 2>(G, V, moved);
        if (!moved) break;
    }
    double sg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sg[c] = sqrt(G[c] * G[c] + G[3 + c] * G[3 + c] + G[6 + c] * G[6 + c]);
    int j = 0;
    if (sg[1] > sg[0]) j = 1;
    if (sg[2] > (j == 0 ? sg[0] : sg[1])) j = 2;
    const double s = j == 0 ? sg[0] : (j == 1 ? sg[1] : sg[2]);
    if (!(s > 0x1p-90 * thin[7])) return false;
    const double u1[3] = {thin[1], thin[2], thin[3]}, v1[3] = {thin[4], thin[5], thin[6]};
    double u2[3], v2[3], du = 0.0, dv = 0.0, nu = 0.0, nv = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) { u2[r] = col3(G, r * 3, j) / s; v2[r] = col3(V, r * 3, j); du += u1[r] * u2[r]; dv += v1[r] * v2[r]; }
#pragma unroll
    for (int r = 0; r < 3; ++r) { u2[r] -= du * u1[r]; v2[r] -= dv * v1[r]; nu += u2[r] * u2[r]; nv += v2[r] * v2[r]; }
    if (!(nu > 0.25 && nv > 0.25)) return false;                       // (rounding noise along u1 / v1: no direction of its own)
    nu = sqrt(nu); nv = sqrt(nv);
#pragma unroll
    for (int r = 0; r < 3; ++r) { u2[r] /= nu; v2[r] /= nv; }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
    return true;
}

// Centred cross-covariance of the nsel selected correspondences and the pose, by ONE wave (all 64 lanes active): nsel is tens to a
// few hundred — lanes stride over them, the 6 + 9 sums are reduced with DPP (no workgroup barrier, no LDS round trip), lane 63's
// totals are broadcast, and every lane forms the same pose in registers (the caller lets one of them store it).
template <typename Fetch>
__device__ __forceinline__ void wave_pose(double (&T)[16], int dim, int nsel, int lane, Fetch&& fetch /* (t, a[3], b[3]): the t-th pair of points */)
{
    constexpr int KEEP = 2;                                     // pairs a lane keeps in registers for the second sweep (128 of them: beyond, the points are fetched again)
    double ka[KEEP][3], kq[KEEP][3];
    double m1[3] = {0, 0, 0}, m2[3] = {0, 0, 0};
#pragma unroll
    for (int x = 0; x < KEEP; ++x) {
        const int t = lane + 64 * x;
        if (t < nsel) fetch(t, ka[x], kq[x]);
        else {
#pragma unroll
            for (int c = 0; c < 3; ++c) { ka[x][c] = 0.0; kq[x][c] = 0.0; }
        }
    }
#pragma unroll
    for (int x = 0; x < KEEP; ++x)
#pragma unroll
        for (int c = 0; c < 3; ++c) { m1[c] += ka[x][c]; m2[c] += kq[x][c]; }
    for (int t = lane + 64 * KEEP; t < nsel; t += 64) {
        double a[3], q[3];
        fetch(t, a, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) { m1[c] += a[c]; m2[c] += q[c]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { m1[c] = readlane63(wave_sum63(m1[c])) / (double)nsel; m2[c] = readlane63(wave_sum63(m2[c])) / (double)nsel; }
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto add = [&](double (&a)[3], double (&q)[3]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] -= m1[c]; q[c] -= m2[c]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) H[r * 3 + c] += a[r] * q[c];
    };
#pragma unroll
    for (int x = 0; x < KEEP; ++x) if (lane + 64 * x < nsel) add(ka[x], kq[x]);
    for (int t = lane + 64 * KEEP; t < nsel; t += 64) {
        double a[3], q[3];
        fetch(t, a, q);
        add(a, q);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) H[e] = readlane63(wave_sum63(H[e]));
    double thin[8];
    thin[0] = 0.0;
    write_pose(T, dim, H, m1, m2, thin);
    if (dim == 3 && thin[0] != 0.0) {                           // rank H <= 1 (the same H in every lane: a uniform branch): a third sweep
        double H2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        auto add2 = [&](const double (&a)[3], const double (&q)[3]) {  // (a, q: centred)
            const double pa = a[0] * thin[1] + a[1] * thin[2] + a[2] * thin[3], pq = q[0] * thin[4] + q[1] * thin[5] + q[2] * thin[6];
            double a2[3], q2[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { a2[c] = a[c] - pa * thin[1 + c]; q2[c] = q[c] - pq * thin[4 + c]; }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) H2[r * 3 + c] += a2[r] * q2[c];
        };
#pragma unroll
        for (int x = 0; x < KEEP; ++x) if (lane + 64 * x < nsel) add2(ka[x], kq[x]);   // (kept pairs were centred in place)
        for (int t = lane + 64 * KEEP; t < nsel; t += 64) {
            double a[3], q[3];
            fetch(t, a, q);
#pragma unroll
            for (int c = 0; c < 3; ++c) { a[c] -= m1[c]; q[c] -= m2[c]; }
            add2(a, q);
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) H2[e] = readlane63(wave_sum63(H2[e]));
        double R[9];
        if (thin_rotation(thin, H2, R)) store_pose(T, dim, R, m1, m2);
    }
}

// Exact emulation of findIndicesOfkLargest (min-heap on (value,index); strict '<' replacement)
// over the FULL association index space (dead associations have u == 0).  Single thread; only
// runs when the k-th largest value is tied or fewer than omega entries are positive.
__device__ inline bool hp_less(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }
__device__ __noinline__ void heap_select_serial(const double* u, const int32_t* lp /* ascending: live order */,
                                   const uint32_t* vecOfLive /* live index -> index into u, or nullptr = identity */,
                                   int L, int nA, int k, bool liveOnly /* removed associations are not candidates at all (pruned list) */,
                                   double* hv, int32_t* hi /* capacity k */, int32_t* outNodesOrig)
{
    int sz = 0, nl = 0;
    const int nIter = liveOnly ? L : nA;
    for (int it = 0; it < nIter; ++it) {
        int p = it; double x = 0.0;
        if (liveOnly) { p = lp[it]; x = u[vecOfLive ? (int)vecOfLive[it] : it]; }
        else if (nl < L && lp[nl] == p) { x = u[vecOfLive ? (int)vecOfLive[nl] : nl]; ++nl; }
        if (sz < k) {
            int c = sz++; hv[c] = x; hi[c] = p;
            while (c > 0) { const int par = (c - 1) >> 1; if (!hp_less(hv[c], hi[c], hv[par], hi[par])) break;
                const double tv = hv[c]; const int ti = hi[c]; hv[c] = hv[par]; hi[c] = hi[par]; hv[par] = tv; hi[par] = ti; c = par; }
        } else if (hv[0] < x) {
            hv[0] = x; hi[0] = p;
            int c = 0;
            for (;;) { int l = 2 * c + 1, r = l + 1, s = c;
                if (l < sz && hp_less(hv[l], hi[l], hv[s], hi[s])) s = l;
                if (r < sz && hp_less(hv[r], hi[r], hv[s], hi[s])) s = r;
                if (s == c) break;
                const double tv = hv[c]; const int ti = hi[c]; hv[c] = hv[s]; hi[c] = hi[s]; hv[s] = tv; hi[s] = ti; c = s; }
        }
    }
    const int kk = sz;
    for (int t = 0; t < kk; ++t) {
        outNodesOrig[kk - t - 1] = hi[0];
        hv[0] = hv[sz - 1]; hi[0] = hi[sz - 1]; --sz;
        int c = 0;
        for (;;) { int l = 2 * c + 1, r = l + 1, s = c;
            if (l < sz && hp_less(hv[l], hi[l], hv[s], hi[s])) s = l;
            if (r < sz && hp_less(hv[r], hi[r], hv[s], hi[s])) s = r;
            if (s == c) break;
            const double tv = hv[c]; const int ti = hi[c]; hv[c] = hv[s]; hi[c] = hi[s]; hv[s] = tv; hi[s] = ti; c = s; }
    }
}

// Tail shared by every solver variant: final u to the row pool, top-omega rounding (with the exact
// heap emulation on ties), selected associations, Umeyama pose, statistics.  `u` is indexed by "vector index":
// the live index (fallback solver) or the position (stream solver); lp[lo + v] is the association index of
// vector index v.  lpAsc is the ascending association list in live order and vecOfLive the live -> vector index
// map (nullptr: identity) — only the sequential heap emulation needs them.  pv / pidx / nodesLive are scratch
// arrays of capacity L.
__device__ __noinline__ void finish_one(const DevParams& D, int b, const ProbDesc& pd, const double* __restrict__ feats,
                                        const int32_t* __restrict__ assoc, const int32_t* __restrict__ lp,
                                        const int32_t* __restrict__ lpAsc, const uint32_t* __restrict__ vecOfLive,
                                        const uint32_t* __restrict__ outIdx /* vector index -> slot of uOut (nullptr: identity) */, const SolveOut& O,
                                        const double* u, double* pv, int32_t* pidx, int32_t* nodesLive,
                                        int L, int rb, int64_t lo, double F, int status, roman_stats_t S,
                                        double* red, int* sint)
{
    const roman_params_t& P = D.p;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int dim = P.point_dim;
    int nsel = 0;
    __syncthreads();
#ifdef ROMAN_SMALL_TIMING
    unsigned long long tf_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; tf_[0] = __builtin_readcyclecounter();
#define FMARK(i_) tf_[i_] = __builtin_readcyclecounter()
#else
#define FMARK(i_) do { } while (0)
#endif
    if (L > 0) {
        // final u to the row pool (stepwise API, tests)
        for (int p = tid; p < L; p += nt) O.uOut[rb + (outIdx ? (int)outIdx[lo + p] : p)] = u[p];

        // ---- top-omega rounding --------------------------------------------------------------
        const double om = round(F);
        int omega = (om >= 2147483647.0) ? 2147483647 : (om < 1.0 ? 0 : (int)om);
        if (omega > (D.pruned ? L : pd.nA)) omega = D.pruned ? L : pd.nA;
        int32_t* nodesOrig = O.nodesOrig + rb;        // capacity L
        if (tid == 0) { sint[0] = 0; sint[1] = 0; }
        __syncthreads();
        if (omega > 0) {
            // compact the positive entries (order irrelevant: ranks below are order-free) as (value, association index)
            // (one LDS atomic per wave and sweep — the wave's count — instead of one per positive element on the same word)
            for (int p0 = 0; p0 < L; p0 += nt) {
                const int p = p0 + tid;
                const double up = p < L ? u[p] : 0.0;
                const unsigned long long pm = __ballot(up > 0.0);
                if (pm) {
                    int base_ = 0;
                    if ((tid & 63) == 0) base_ = atomicAdd(&sint[0], (int)__popcll(pm));
                    base_ = __builtin_amdgcn_readfirstlane(base_);
                    if (up > 0.0) {
                        const int pos = base_ + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
                        pv[pos] = up; pidx[pos] = lp[lo + p];
                    }
                }
            }
            __syncthreads();
            FMARK(1);
            const int Pn = sint[0];
            bool fallback = (Pn < omega) || (omega > L);
            if (!fallback) {
                // rank of e = number of entries greater in (value, association index) order (the inner loop reads LDS only)
                // `parts` adjacent lanes share an entry (a power of two, as many as the threads allow: a hundred entries leave four fifths
                // of a 512-thread workgroup idle otherwise), each counts a part of the list, a butterfly inside the group adds the counts
                int parts = 1;
                while (parts < 8 && 2 * parts * Pn <= nt) parts <<= 1;
                const int chunk = (Pn + parts - 1) / parts;
                for (int base = 0; base < Pn * parts; base += nt) {
                    const int idx = base + tid, e = idx / parts, part = idx & (parts - 1);
                    const bool act = e < Pn;
                    const double ve = pv[act ? e : 0]; const int ae = pidx[act ? e : 0];
                    const int flo = part * chunk, fhi = min(Pn, flo + chunk);
                    int rank = 0;
                    for (int f0 = flo; f0 < fhi; f0 += 8) {         // eight LDS reads in flight (one per iteration: the loop ran at the LDS latency)
                        double vf[8]; int af[8];
#pragma unroll
                        for (int x = 0; x < 8; ++x) { const int f2 = min(f0 + x, Pn - 1); vf[x] = pv[f2]; af[x] = pidx[f2]; }
#pragma unroll
                        for (int x = 0; x < 8; ++x) rank += (f0 + x < fhi && ((vf[x] > ve) || (vf[x] == ve && af[x] > ae))) ? 1 : 0;
                    }
                    for (int off = 1; off < parts; off <<= 1) rank += __shfl_xor(rank, off);
                    if (act && part == 0) {
                        if (rank < omega) nodesLive[rank] = ae;
                        if (rank == omega - 1) { red[64] = ve; }
                    }
                }
                __syncthreads();
                FMARK(2);
                // a tie at the cut: an entry as large as the omega-th one ranks behind it <=> more than omega entries are >= that value
                const double vstar = red[64];
                int ge = 0;
                for (int e = tid; e < Pn; e += nt) ge += (pv[e] >= vstar) ? 1 : 0;
                if (ge) atomicAdd(&sint[1], ge);
                __syncthreads();
                fallback = sint[1] > omega;
            }
            if (fallback) {
                status |= ROMAN_ST_TIE_FALLBACK;
                __syncthreads();
                if (tid == 0) {
                    const int kk = min(omega, L);      // heap capacity bounded by the scratch size
                    heap_select_serial(u, lpAsc + lo, vecOfLive ? vecOfLive + lo : nullptr, L, pd.nA, kk, D.pruned != 0, pv, pidx, nodesOrig);
                    sint[0] = kk;
                }
                __syncthreads();
                nsel = sint[0];
            } else {
                nsel = omega;
                for (int t = tid; t < nsel; t += nt) nodesOrig[t] = nodesLive[t];
            }
            __syncthreads();
        }
    }

    FMARK(3);
    // ---- outputs: associations, pose, stats ------------------------------------------------------
    const int32_t* nodesOrigR = O.nodesOrig + rb;
    const int kout = min(nsel, O.kmax);
    if (nsel > O.kmax) status |= ROMAN_ST_ASSOC_TRUNCATED;
    for (int t = tid; t < kout; t += nt) {
        int i, j;
        decode_assoc(pd, assoc, nodesOrigR[t], i, j);
        O.assoc_out[((int64_t)b * O.kmax + t) * 2 + 0] = i;
        O.assoc_out[((int64_t)b * O.kmax + t) * 2 + 1] = j;
    }
    FMARK(4);
    // pose from ALL selected associations ([REF object_registration.py:110-128], unit weights)
    double Tp[16];
    bool have_pose = false;
    if (nsel >= dim && feats != nullptr && !(status & ROMAN_ST_EMPTY_MAP)) {
        if (tid < 64) {                                         // (wave 0: wave_pose)
            wave_pose(Tp, dim, nsel, tid, [&](int t, double (&a)[3], double (&q)[3]) {
                int i, j;
                decode_assoc(pd, assoc, nodesOrigR[t], i, j);
                const double* pa = feats + (pd.off1 + i) * D.F; const double* pb = feats + (pd.off2 + j) * D.F;
#pragma unroll
                for (int c = 0; c < 3; ++c) { a[c] = c < dim ? pa[c] : 0.0; q[c] = c < dim ? pb[c] : 0.0; }
            });
        }
        FMARK(5);
        FMARK(6);
        have_pose = true;
    } else {
        status |= ROMAN_ST_INSUFFICIENT;
    }
    if (tid == 0) {
        for (int t = 0; t < 16; ++t) O.T_out[(int64_t)b * 16 + t] = have_pose ? Tp[t] : d_nan();
        O.n_assoc_out[b] = kout;
        O.status_out[b] = status;
        O.nSel[b] = nsel;
        if (O.stats_out) O.stats_out[b] = S;
    }
    __syncthreads();
#ifdef ROMAN_SMALL_TIMING
    FMARK(7);
    if (tid == 0 && ((b & 255) == 0 || b < 2)) printf("[finish_one nt=%d] b=%d L=%d nsel=%d cycles: compact %llu ranks %llu ties %llu outputs %llu sums %llu rotation %llu write %llu\n", nt, b, L, nsel,
                                                       tf_[1] - tf_[0], tf_[2] - tf_[1], tf_[3] - tf_[2], tf_[4] - tf_[3], tf_[5] - tf_[4], tf_[6] - tf_[5], tf_[7] - tf_[6]);
#endif
#undef FMARK
}


/*
 * solve_one: CLIPPER findDenseClique on one problem, by one workgroup (k_solve: many mid-size problems of the fallback
 * kind; few large ones go to k_solve_wide, the whole device on one problem).
 * Mirrors oracle_solve() step for step (see there for the restated upstream algorithm):
 * gradF is never stored: it is recombined on the fly from (u, Mu, Cu, d, sum u), bitwise the same
 * value the oracle keeps in its gradF vector.
 */
// MODE 2: u, u_new, Mu, Cu, Mu_new, Cu_new and the diagonal all live in LDS (7 * Lcap doubles);
// MODE 1: only u and u_new (the gathered vectors) do, the row vectors sit in the L2-resident pools;
// MODE 0: nothing fits, everything is in the pools.
template <typename IdxT, int MODE>
__device__ void solve_one(const DevParams& D, int b, const ProbDesc& pd, ProbState* st,
                          const double* __restrict__ feats, const int32_t* __restrict__ assoc,
                          const int32_t* __restrict__ lp, const double* __restrict__ ls,
                          const uint32_t* __restrict__ permPool, const uint32_t* __restrict__ rowPosPool,
                          const uint32_t* __restrict__ sliceWidthPool, const uint32_t* __restrict__ sliceBasePool,
                          const IdxT* __restrict__ colsPool, const double* __restrict__ valsPool,
                          double* __restrict__ vMu, double* __restrict__ vCu,
                          double* __restrict__ vMun, double* __restrict__ vCun,
                          double* __restrict__ gU, double* __restrict__ gUn,
                          int32_t* __restrict__ plpPool /* position -> association index */, double* __restrict__ pldPool /* diagonal by position */,
                          const double* __restrict__ u0, const SolveOut& O,
                          double* sv /* LDS vectors */, int Lcap, double* red, int* sint)
{
    // Every vector is indexed by POSITION (the sorted row order of the layout; the matrix's column labels are positions):
    // element p belongs to the live association perm[p].
    const roman_params_t& P = D.p;
    const int ltid = threadIdx.x, nw = blockDim.x >> 6;
    const int nt = (int)blockDim.x;
    const int tid = ltid;
#define SUM2(a_, b_) block_sum2(a_, b_, red, par, ltid, nw)
    const int L = st[b].L, rb = st[b].rowBase;
    const int64_t lo = pd.liveOff;
    const uint32_t* perm = permPool + lo; const uint32_t* swid = sliceWidthPool + lo; const uint32_t* sbase = sliceBasePool + lo;
    const IdxT* cols = colsPool + st[b].nnzOff; const double* vals = valsPool + st[b].nnzOff;
    double* u = (MODE >= 1) ? sv : gU + rb;
    double* un = (MODE >= 1) ? sv + Lcap : gUn + rb;
    double* Mu = (MODE == 2) ? sv + 2 * Lcap : vMu + rb;
    double* Cu = (MODE == 2) ? sv + 3 * Lcap : vCu + rb;
    double* Mun = (MODE == 2) ? sv + 4 * Lcap : vMun + rb;
    double* Cun = (MODE == 2) ? sv + 5 * Lcap : vCun + rb;
    int32_t* plp = plpPool + lo; double* pld = pldPool + lo;
    for (int p = tid; p < L; p += nt) { const uint32_t k_ = perm[p]; plp[p] = lp[lo + k_]; pld[p] = ls[lo + k_]; }
    __syncthreads();
    const double* sd = pld;                           // diagonal M_pp = single score
    if (MODE == 2) {
        double* sdl = sv + 6 * Lcap;
        for (int p = tid; p < L; p += nt) sdl[p] = pld[p];
        sd = sdl;
    }

    int par = 0;

    int status = ROMAN_ST_OK;
    roman_stats_t S;
    S.n_assoc_in = pd.nA; S.n_live = L; S.nnz_upper = (int64_t)st[b].nnzUpper;
    S.n_pass = 0; S.outer_iters = 0; S.inner_iters = 0; S.ls_trials = 0; S.score = 0.0; S.d_final = 0.0;
    double F = 0.0, d = 0.0;

    if (pd.n1 == 0 || pd.n2 == 0) status |= ROMAN_ST_EMPTY_MAP;
    if (L > 0) {
        // ---- initialisation: u = normalize(M u0 + diag u0) ------------------------------------
        for (int p = tid; p < L; p += nt) u[p] = u0 ? u0[lo + plp[p]] : 1.0;
        __syncthreads();
        if (P.rescale_u0) {
            spmv_sell<IdxT, 4>(u, L, perm, swid, sbase, cols, vals, Mu, Cu, tid, nt); ++S.n_pass;
            __syncthreads();
            for (int p = tid; p < L; p += nt) u[p] = Mu[p] + sd[p] * u[p];
            __syncthreads();
        }
        {
            double ss = 0.0, dummy = 0.0;
            for (int p = tid; p < L; p += nt) ss += u[p] * u[p];
            SUM2(ss, dummy);
            const double nr = sqrt(ss);
            if (nr > 0.0) for (int p = tid; p < L; p += nt) u[p] /= nr;
            __syncthreads();
        }
        spmv_sell<IdxT, 4>(u, L, perm, swid, sbase, cols, vals, Mu, Cu, tid, nt); ++S.n_pass;
        double usum = 0.0;
        { double dummy = 0.0; for (int p = tid; p < L; p += nt) usum += u[p]; SUM2(usum, dummy); }
        // the barrier inside block_sum2 also orders the Mu/Cu stores of spmv_sell before the reads below
        {   // initial d: signed mean of (Mu)_p / Cbu_p over the active set
            double acc = 0.0, cnt = 0.0;
            for (int p = tid; p < L; p += nt) {
                const double up = u[p], Cbu = (usum - Cu[p]) - up;
                if (Cbu > P.eps && up > P.eps) { acc += (Mu[p] + sd[p] * up) / Cbu; cnt += 1.0; }
            }
            SUM2(acc, cnt);
            d = (cnt > 0.0) ? acc / cnt : 0.0;
        }
        // ---- projected gradient ascent with homotopy on d ---------------------------------------
        int i;
        for (i = 0; i < P.maxoliters; ++i) {
            {
                double f = 0.0, dummy = 0.0;
                for (int p = tid; p < L; p += nt) {
                    const double up = u[p];
                    const double g = (((sd[p] + d) * up - d * usum) + Mu[p]) + Cu[p] * d;
                    f += up * g;
                }
                SUM2(f, dummy);
                F = f;
            }
            for (int j = 0; j < P.maxiniters; ++j) {
                double alpha = 1.0, Fnew = 0.0, deltaF = 0.0, unsum = 0.0, du2 = 0.0;
                for (int k = 0; k < P.maxlsiters; ++k) {
                    double ss = 0.0, dummy = 0.0;
                    for (int p = tid; p < L; p += nt) {
                        const double up = u[p];
                        const double g = (((sd[p] + d) * up - d * usum) + Mu[p]) + Cu[p] * d;
                        double t = up + alpha * g;
                        t = t > 0.0 ? t : 0.0;
                        un[p] = t; ss += t * t;
                    }
                    SUM2(ss, dummy);
                    const double nr = sqrt(ss);
                    double s1 = 0.0, dd = 0.0;
                    for (int p = tid; p < L; p += nt) {
                        double t = un[p];
                        if (nr > 0.0) { t /= nr; un[p] = t; }
                        s1 += t;
                        const double df = t - u[p]; dd += df * df;
                    }
                    SUM2(s1, dd);
                    unsum = s1; du2 = dd;
                    spmv_sell<IdxT, 4>(un, L, perm, swid, sbase, cols, vals, Mun, Cun, tid, nt); ++S.n_pass; ++S.ls_trials;
                    __syncthreads();
                    double f = 0.0;
                    for (int p = tid; p < L; p += nt) {
                        const double up = un[p];
                        const double g = (((sd[p] + d) * up - d * unsum) + Mun[p]) + Cun[p] * d;
                        f += up * g;
                    }
                    SUM2(f, dummy);
                    Fnew = f;
                    deltaF = Fnew - F;
                    if (deltaF < -P.eps) alpha *= P.beta; else break;
                }
                const double du = sqrt(du2);
                F = Fnew; usum = unsum;
                { double* t; t = u; u = un; un = t; t = Mu; Mu = Mun; Mun = t; t = Cu; Cu = Cun; Cun = t; }
                ++S.inner_iters;
                if (du < P.tol_u || fabs(deltaF) < P.tol_F) break;
            }
            double acc = 0.0, cnt = 0.0;
            for (int p = tid; p < L; p += nt) {
                const double up = u[p], Cbu = (usum - Cu[p]) - up;
                if (Cbu > P.eps && up > P.eps) { acc += fabs((Mu[p] + sd[p] * up) / Cbu); cnt += 1.0; }
            }
            SUM2(acc, cnt);
            if (cnt > 0.0) d += acc / cnt; else break;
        }
        if (i >= P.maxoliters) status |= ROMAN_ST_MAXITER;
        S.outer_iters = i; S.score = F; S.d_final = d;

        __syncthreads();                         // every element of the final u is in memory
        finish_one(D, b, pd, feats, assoc, plpPool, lp, rowPosPool, permPool, O, u, Mun, (int32_t*)un, (int32_t*)Cun, L, rb, lo, F, status, S, red, sint);
        return;
    }
    finish_one(D, b, pd, feats, assoc, plpPool, lp, rowPosPool, permPool, O, nullptr, nullptr, nullptr, nullptr, L, rb, lo, F, status, S, red, sint);
#undef SUM2
}


template <typename IdxT, int MODE>
__global__ void __launch_bounds__(1024) k_solve(DevParams D, int B, const ProbDesc* __restrict__ probs,
                                                ProbState* __restrict__ st,
                                                const double* __restrict__ feats, const int32_t* __restrict__ assoc,
                                                const int32_t* __restrict__ lp, const double* __restrict__ ls,
                                                const uint32_t* __restrict__ perm, const uint32_t* __restrict__ rowPos,
                                                const uint32_t* __restrict__ sliceWidth, const uint32_t* __restrict__ sliceBase,
                                                const IdxT* __restrict__ cols, const double* __restrict__ vals,
                                                double* __restrict__ vMu, double* __restrict__ vCu,
                                                double* __restrict__ vMun, double* __restrict__ vCun,
                                                double* __restrict__ gU, double* __restrict__ gUn,
                                                int32_t* __restrict__ plp, double* __restrict__ pld,
                                                const double* __restrict__ u0, SolveOut O,
                                                int* __restrict__ queue, int Lcap)
{
    // LDS: [MODE 2: 7 | MODE 1: 2 | MODE 0: 0] vectors of Lcap doubles, 72 doubles of reduction
    // scratch (2 x 32 ping-pong + 8), 4 ints
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NVEC = (MODE == 2) ? 7 : (MODE == 1 ? 2 : 0);
    double* sv = reinterpret_cast<double*>(smem);
    double* red = sv + (size_t)NVEC * Lcap;
    int* sint = reinterpret_cast<int*>(red + 72);
    for (;;) {
        if (threadIdx.x == 0) sint[2] = atomicAdd(queue, 1);
        __syncthreads();
        const int b = __builtin_amdgcn_readfirstlane(sint[2]);
        __syncthreads();
        if (b >= B) break;
        if (__builtin_amdgcn_readfirstlane(st[b].kind) == 1) {   // (else: the stream solver's problem, or a skipped one)
            const ProbDesc pd = probs[b];
            if (MODE > 0 && st[b].L <= Lcap)
                solve_one<IdxT, MODE>(D, b, pd, st, feats, assoc, lp, ls, perm, rowPos, sliceWidth, sliceBase, cols, vals,
                                      vMu, vCu, vMun, vCun, gU, gUn, plp, pld, u0, O, sv, Lcap, red, sint);
            else
                solve_one<IdxT, 0>(D, b, pd, st, feats, assoc, lp, ls, perm, rowPos, sliceWidth, sliceBase, cols, vals,
                                   vMu, vCu, vMun, vCun, gU, gUn, plp, pld, u0, O, sv, Lcap, red, sint);
        }
    }
}

#ifdef ROMAN_SOLVE_TIMING
#define TMARK(slot) do { const unsigned long long t__ = __builtin_readcyclecounter(); tacc[slot] += t__ - tlast; tcnt[slot] += 1; tlast = t__; } while (0)
#else
#define TMARK(slot) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// Stream solver (kind 0: L <= STREAM_MAXL, 16-bit position indices, upper-triangle quad layout).
//
// One workgroup of NW waves per problem.  Thread t OWNS the vector elements p = t, t + NT, t + 2 NT (positions):
// u, M u, C u, the diagonal and the trial vector with its products live in that thread's registers.  LDS holds
// only what the SpMV touches by index: the vector being multiplied (xg) and two accumulator arrays.
//
// SpMV on the upper triangle, pull + push.  A stored entry (p, q, v), p < q, serves both triangles:
//      (M x)_p += v x_q      pulled: the row's lane gathers x_q from LDS and accumulates in registers,
//      (M x)_q += v x_p      pushed: an LDS atomic add into the accumulator of q,
// and likewise (C x) with v replaced by 1.  Every pass therefore moves 10 bytes per non-zero of the UPPER
// triangle, and — positions being ranks by degree — a vector whose support lies in the first S slices needs only
// those S slices: rows beyond have x_p = 0 (nothing to push) and only columns q > p beyond the support (nothing
// to pull).  The solver's long tail runs on the clique found so far, i.e. on the first one or two slices; no
// column-compacted copies of the matrix are needed.
//
// Exact accumulation.  Atomic floating-point adds would make the sums depend on the order in which waves reach
// the LDS.  Every term is instead rounded ONCE to a fixed-point integer, rint(v x 2^s) (s chosen per pass from
// max x so that a term is below 2^49 and any sum below 2^62), and integers are added — in registers for the
// pulled part, with ds_add_u64 for the pushed part and for the flush of a row's pulled sum.  Integer addition is
// associative: the result does not depend on the order, on the number of waves, or on how the stream is split.
// The rounding unit 2^-s is 2^-48 relative to the largest element of x, the same order as the rounding of an f64
// summation.  The conversion is one fma against 2^52 + 2^51 (the integer appears in the low mantissa bits).
//
// Fused passes (round 5).  Inside the line search only the sum (M + d C) x enters the gradient; M x and C x are needed
// apart only where d itself is updated (once per outer iteration).  A line-search pass therefore accumulates ONE
// fixed-point sum per element with the weight v + d (v alone where C_pq = 0): one LDS gather and ONE ds_add_u64 per
// stored pair instead of one and two; the d update is preceded by a SPLIT pass (both sums) over the accepted vector.
// The same order is stated in the oracle (oracle_set_pass_mode(1), its default).
//
// One balanced stream: the S slices of a pass are contiguous in memory (quads); wave w streams the quads
// [w T / NW, (w+1) T / NW) with ST_D quads (9 wide loads) in flight per lane, whatever slices the range covers
// (lane = row slot of the current slice) and flushes its pulled sums when it leaves a slice or its range.
// ---------------------------------------------------------------------------------------------
constexpr int SOLVE_WAVES = 8;           // waves of the stream solver's workgroup (one problem per workgroup; measured: 8 beats 16, and beats 4)
constexpr int ST_D = 3;                  // quads in flight per lane
constexpr int ST_MAXSL = STREAM_MAXL / 64;
constexpr int SMALL_MAXL = 128;           // live associations the one-wave-per-problem instantiation of k_solve_up takes
constexpr int COO_E = 6;                  // one-wave instantiation: stored pairs a lane holds in registers (coordinate form)
constexpr int COO_CAP = 64 * COO_E;       // ... per problem; larger matrices take the quad stream
constexpr uint32_t ST_CZ = 0x8000u, ST_MASK = 0x7fffu;
constexpr unsigned long long FX_MAGIC_BITS = 0x4338000000000000ull;     // 2^52 + 2^51
#define FX_MAGIC 6755399441055744.0

// Explicit address spaces for the hot pointers of the stream: FLAT accesses would count against lgkmcnt as well and
// every wait for an LDS gather would drain the prefetched matrix loads.
#define ROMAN_GLOBAL __attribute__((address_space(1)))
#define ROMAN_LDS __attribute__((address_space(3)))
typedef const ROMAN_GLOBAL unsigned long long* g_quad_cp;    // 4 x u16 column indices of one lane
typedef const ROMAN_GLOBAL dbl2_t* g_pair_cp;                // 2 x f64 values of one lane
typedef const ROMAN_LDS double* l_vec_cp;                    // gathered vector in LDS
typedef ROMAN_LDS unsigned long long* l_acc_p;               // fixed-point accumulators in LDS

// wave-uniform values that the compiler cannot prove uniform (read from LDS, derived from threadIdx):
// force them into SGPRs so that loop control and matrix addressing run on the scalar unit
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane((int)b), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_mov(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROWMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROWMASK, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// sum / maximum (of non-negative values) over the 64 lanes, valid in lane 63 (fixed tree: pairs, quads, rows of 16,
// then across rows; rows a row_bcast does not reach receive 0, the neutral element of both)
__device__ __forceinline__ double wave_sum63(double v)
{
    v += dpp_mov<0xB1, 0xf>(v);          // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E, 0xf>(v);          // quad_perm [2,3,0,1]
    v += dpp_mov<0x124, 0xf>(v);         // row_ror:4
    v += dpp_mov<0x128, 0xf>(v);         // row_ror:8
    v += dpp_mov<0x142, 0xa>(v);         // row_bcast:15 -> rows 1,3
    v += dpp_mov<0x143, 0xc>(v);         // row_bcast:31 -> rows 2,3
    return v;
}
__device__ __forceinline__ double wave_max63(double v)
{
    v = fmax(v, dpp_mov<0xB1, 0xf>(v));
    v = fmax(v, dpp_mov<0x4E, 0xf>(v));
    v = fmax(v, dpp_mov<0x124, 0xf>(v));
    v = fmax(v, dpp_mov<0x128, 0xf>(v));
    v = fmax(v, dpp_mov<0x142, 0xa>(v));
    v = fmax(v, dpp_mov<0x143, 0xc>(v));
    return v;
}
__device__ __forceinline__ double readlane63(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// NS sums and NM maxima (of non-negative values) over the NW waves of the block, identical in every thread; fixed
// reduction tree.  `red`: two ping-pong areas of NW*8 doubles (a buffer is rewritten only after the barrier of the
// next call).  The barrier inside also publishes whatever the caller wrote to LDS before the call.
constexpr int RED_STRIDE = 8;
// doubles of reduction scratch a stream-solver workgroup of NW waves owns: the solver's ping-pong areas, and at least the 72 that
// finish_one() uses whatever the workgroup size (two areas of 32 + the slot red[64]).  (With 2 * NW * RED_STRIDE + 8 = 24 the
// one-wave instantiation wrote red[32..33] over its unused slice table and red[64] BEHIND its LDS allocation.)
constexpr int red_doubles(int NW) { return 2 * NW * RED_STRIDE + 8 > 72 ? 2 * NW * RED_STRIDE + 8 : 72; }
template <int NW, int NS, int NM>
__device__ __forceinline__ void block_red(double (&sv)[NS > 0 ? NS : 1], double (&mv)[NM > 0 ? NM : 1], double* red, int& par, int tid)
{
    static_assert(NS + NM <= RED_STRIDE, "reduction scratch");
    static_assert(NW == 1 || NW == 4 || NW == 8 || NW == 16, "cross-wave butterfly");
    if (NW == 1) {                                              // a single wave: the wave reduction is the block reduction
#pragma unroll
        for (int i = 0; i < NS; ++i) sv[i] = uni(readlane63(wave_sum63(sv[i])));
#pragma unroll
        for (int i = 0; i < NM; ++i) mv[i] = uni(readlane63(wave_max63(mv[i])));
        __syncthreads();                                        // (publishes the caller's LDS writes like the general path; one wave: no wait)
        return;
    }
    double* rr = red + NW * RED_STRIDE * par;
    par ^= 1;
    const int w = uni(tid >> 6);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double s = readlane63(wave_sum63(sv[i]));
        if ((tid & 63) == 0) rr[RED_STRIDE * w + i] = s;
    }
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        const double m = readlane63(wave_max63(mv[i]));
        if ((tid & 63) == 0) rr[RED_STRIDE * w + NS + i] = m;
    }
    __syncthreads();
    // cross-wave step: lane l takes the partial of wave l % NW; the NW lanes of a DPP row are combined with a fixed
    // butterfly (every lane ends with the total), the result moves to an SGPR
    const int src = (tid & 63) & (NW - 1);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double v = rr[RED_STRIDE * src + i];
        v += dpp_mov<0xB1, 0xf>(v);          // quad_perm [1,0,3,2]
        v += dpp_mov<0x4E, 0xf>(v);          // quad_perm [2,3,0,1]
        if (NW > 4) v += dpp_mov<0x124, 0xf>(v);         // row_ror:4
        if (NW > 8) v += dpp_mov<0x128, 0xf>(v);     // row_ror:8
        sv[i] = uni(v);
    }
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        double v = rr[RED_STRIDE * src + NS + i];
        v = fmax(v, dpp_mov<0xB1, 0xf>(v));
        v = fmax(v, dpp_mov<0x4E, 0xf>(v));
        if (NW > 4) v = fmax(v, dpp_mov<0x124, 0xf>(v));
        if (NW > 8) v = fmax(v, dpp_mov<0x128, 0xf>(v));
        mv[i] = uni(v);
    }
}

// The same reduction of NS sums in two halves, for a result that is not needed before the caller's NEXT workgroup barrier anyway:
// block_post() leaves every wave's partial in the ping-pong area (no barrier), block_collect() — behind any later __syncthreads()
// of the caller, and before the second block_red() / block_post() after the post — finishes it.  Same tree, same bits as block_red().
template <int NW, int NS>
__device__ __forceinline__ const double* block_post(const double (&sv)[NS], double* red, int& par, int tid)
{
    static_assert(NW == 4 || NW == 8 || NW == 16, "cross-wave butterfly");
    double* rr = red + NW * RED_STRIDE * par;
    par ^= 1;
    const int w = uni(tid >> 6);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double s = readlane63(wave_sum63(sv[i]));
        if ((tid & 63) == 0) rr[RED_STRIDE * w + i] = s;
    }
    return rr;
}
template <int NW, int NS>
__device__ __forceinline__ void block_collect(double (&sv)[NS], const double* rr, int tid)
{
    const int src = (tid & 63) & (NW - 1);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double v = rr[RED_STRIDE * src + i];
        v += dpp_mov<0xB1, 0xf>(v);          // quad_perm [1,0,3,2]
        v += dpp_mov<0x4E, 0xf>(v);          // quad_perm [2,3,0,1]
        if (NW > 4) v += dpp_mov<0x124, 0xf>(v);         // row_ror:4
        if (NW > 8) v += dpp_mov<0x128, 0xf>(v);     // row_ror:8
        sv[i] = uni(v);
    }
}

// fixed-point accumulator -> double (the accumulated integer is below 2^62)
__device__ __forceinline__ double fx_decode(unsigned long long a, double inv)
{
    return fma((double)(uint32_t)(a >> 32), 4294967296.0, (double)(uint32_t)a) * inv;
}

template <int NW, bool HASCZ, int MAXL, bool COOONLY = false /* the matrix is ALWAYS a pre-built coordinate list (k_small): no quad stream in the code */>
__device__ void solve_up(const DevParams& D, int b, const ProbDesc& pd, ProbState* st,
                         const double* __restrict__ feats, const int32_t* __restrict__ assoc,
                         const int32_t* __restrict__ plp /* position -> association index */, const int32_t* __restrict__ lpAsc,
                         const uint32_t* __restrict__ rowPosPool, const double* __restrict__ pld /* diagonal, position order */,
                         const uint32_t* __restrict__ sliceBasePool,
                         const uint16_t* __restrict__ colsPool, const double* __restrict__ valsPool,
                         const double* __restrict__ u0, const SolveOut& O,
                         double* xg /* [Lc] */, unsigned long long* accM /* [Lc] */, unsigned long long* accC /* [Lc] */, int Lc,
                         uint32_t* cumQ /* [ST_MAXSL + 1] */, double* red, int* sint, unsigned char* cooLds /* one-wave instantiation: COO_CAP * 12 bytes */,
                         int cooPre = -1 /* >= 0: cooLds already holds that many entries (k_small); no quad layout exists for the problem */,
                         int rbPre = -1 /* >= 0: offset of the problem in the row pools (k_small runs before k_rowbase) */)
{
    constexpr int NT = NW * 64;
#ifdef ROMAN_SOLVE_TIMING
    const unsigned long long tentry_ = __builtin_readcyclecounter();
#endif
#ifdef ROMAN_SMALL_TIMING
    const unsigned long long tw0_ = wall_clock64();
#endif
    constexpr int KMAX = (MAXL + NT - 1) / NT;                 // elements per thread (the kernel takes problems of up to MAXL live associations)
    // The three LDS vectors lie at a FIXED distance from each other — accM == xg + LCAP, accC == xg + 2 LCAP (the callers lay them
    // out so; Lc == LCAP) —: the stream addresses the accumulators of a column through the column's gather address + an immediate
    constexpr int LCAP = MAXL + 64;
    const roman_params_t& P = D.p;
    // the solver's parameters as scalars (the argument block sits in scratch memory: its address is taken for the shared tail)
    const double p_eps = uni(P.eps), p_beta = uni(P.beta), p_tol_u = uni(P.tol_u), p_tol_F = uni(P.tol_F);
    const int p_maxin = uni(P.maxiniters), p_maxout = uni(P.maxoliters), p_maxls = uni(P.maxlsiters), p_rescale = uni(P.rescale_u0);
    const int tid = threadIdx.x, lane = tid & 63, w = uni(tid >> 6);
    // FOR_K: the thread's elements; in the one-wave instantiation only those that exist in THIS problem (k < ceil(L / 64): a problem
    // of 60 live associations uses one of the two element slots — the other is zero and stays zero, its half of the element-wise
    // work, the bulk of a pass at this size, is skipped; in the general instantiation the same guard costs 20 registers and
    // buys a sixth of 8 % of the time: not applied).  FOR_K_ALL: every slot (initialisation)
#define FOR_K_ALL(k_, p_) _Pragma("unroll") for (int k_ = 0; k_ < KMAX; ++k_) if ([[maybe_unused]] const int p_ = tid + k_ * NT; true)
#define FOR_K(k_, p_) _Pragma("unroll") for (int k_ = 0; k_ < KMAX; ++k_) if ([[maybe_unused]] const int p_ = tid + k_ * NT; NW != 1 || k_ < kUsed)
    const int L = uni(st[b].L), rb = rbPre >= 0 ? rbPre : uni(st[b].rowBase);
    const int kUsed = uni((L + NT - 1) / NT);
    const int64_t lo = pd.liveOff;
    const int nsl = (L + 63) >> 6;
    int par = 0;

    int status = ROMAN_ST_OK;
    roman_stats_t S;
    S.n_assoc_in = pd.nA; S.n_live = L; S.nnz_upper = (int64_t)st[b].nnzUpper;
    S.n_pass = 0; S.outer_iters = 0; S.inner_iters = 0; S.ls_trials = 0; S.score = 0.0; S.d_final = 0.0;
    int n_pass = 0, ls_trials = 0, inner_iters = 0;
    double F = 0.0, d = 0.0;
    if (pd.n1 == 0 || pd.n2 == 0) status |= ROMAN_ST_EMPTY_MAP;
    if (L <= 0) {
        finish_one(D, b, pd, feats, assoc, plp, lpAsc, rowPosPool, nullptr, O, nullptr, nullptr, nullptr, nullptr, L, rb, lo, F, status, S, red, sint);
        return;
    }
#ifdef ROMAN_SOLVE_TIMING
    unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tcnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tlast = __builtin_readcyclecounter();
#endif
    g_quad_cp cbase = (g_quad_cp)(colsPool + st[b].nnzOff) + lane;
    g_pair_cp vbase = (g_pair_cp)(valsPool + st[b].nnzOff) + lane;
    l_vec_cp xl = (l_vec_cp)xg;
    l_acc_p aM = (l_acc_p)accM; l_acc_p aC = (l_acc_p)accC;

    // ---- per-problem set-up: quad prefix of the slices, owned elements, clean LDS --------------------------
    __syncthreads();
    // slice table: lane s of every wave holds the first quad of slice s (lane nsl: the total), read with v_readlane
    const uint32_t cqv = cooPre >= 0 ? 0u : ((lane < nsl) ? (sliceBasePool[lo + lane] >> 8) : (st[b].nnzCap >> 8));
#define CUMQ(s_) ((uint32_t)__builtin_amdgcn_readlane((int)cqv, (s_)))
    for (int p = tid; p < Lc; p += NT) { xg[p] = 0.0; accM[p] = 0ull; accC[p] = 0ull; }
    // Wu: the fused product (M + d C) u of the current u at the current d; Mn / Cn: the products of the pass just done —
    // a fused pass leaves (M + d C) x in Mn and nothing in Cn, a split pass M x and C x
    double u[KMAX], Wu[KMAX], sd[KMAX], tk[KMAX], Mn[KMAX], Cn[KMAX];
    FOR_K_ALL(k, p) {
        const bool in = p < L;
        sd[k] = in ? pld[lo + p] : 0.0;
        u[k] = in ? (u0 ? u0[lo + plp[lo + p]] : 1.0) : 0.0;
        Wu[k] = tk[k] = Mn[k] = Cn[k] = 0.0;
    }
    __syncthreads();

    // ---- one-wave instantiation: the matrix as a COORDINATE list in registers ----------------------------------------
    // A problem of the reference's demo scale has ~60 live associations and ~140 stored pairs; its one slice of 64 rows is
    // as wide as its longest row, so those 140 entries occupy ~1500 slots of the quad layout, and every pass walks them all.
    // The wave compacts the real entries once (ballot ranks, through LDS) into COO_E registers per lane — (row, column, flag)
    // in one word + the value — and a pass is COO_E rounds of two gathers and four pushes, no memory traffic at all.  The sums
    // are the same integers in another order: identical bits.  More than 64 * COO_E stored pairs: the quad stream below.
    [[maybe_unused]] uint32_t cpq[COO_E]; [[maybe_unused]] double cv[COO_E];
    [[maybe_unused]] int cooRounds = -1;                       // -1: not in use
    if constexpr (NW == 1) {
        uint32_t* lpq = reinterpret_cast<uint32_t*>(cooLds); double* lv = reinterpret_cast<double*>(cooLds + 4 * COO_CAP);
        const uint32_t Tq = CUMQ(nsl);
        const uint32_t q1 = nsl > 1 ? CUMQ(1) : Tq;             // (L <= 128: at most two slices)
        uint32_t cnt = 0;
        if (cooPre >= 0) {                                      // the caller (k_small) compacted the entries itself
            cnt = (uint32_t)cooPre;
            cooRounds = (int)((cnt + 63u) >> 6);
#pragma unroll
            for (int e = 0; e < COO_E; ++e) {
                // (lane l holds the CONSECUTIVE entries l R .. l R + R - 1: the list is row-major, so the 64 lanes of a round
                //  push onto 64 different rows instead of onto the few rows 64 consecutive entries belong to)
                const uint32_t at = (uint32_t)lane * (uint32_t)cooRounds + (uint32_t)e;
                const bool have = e < cooRounds && at < cnt;
                const uint32_t dummy = (uint32_t)L + (uint32_t)lane;
                cpq[e] = have ? lpq[at] : (dummy | (dummy << 8) | 0x10000u);
                cv[e] = have ? lv[at] : 0.0;
            }
            __syncthreads();
        } else
        if (!COOONLY && (unsigned long long)st[b].nnzUpper <= (unsigned long long)COO_CAP && nsl <= 2) {
            for (uint32_t qq = 0; qq < Tq; ++qq) {
                const unsigned long long cw = cbase[(size_t)qq * 64];
                const dbl2_t v0 = vbase[(size_t)(2 * qq) * 64], v1 = vbase[(size_t)(2 * qq + 1) * 64];
                const uint32_t row = (qq >= q1 ? 64u : 0u) + (uint32_t)lane;
                const double v4[4] = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t lab = (uint32_t)(cw >> (16 * e)) & 0xffffu, col = lab & ST_MASK;
                    const bool real = col < (uint32_t)L;        // (padding points at the dummy elements L + lane)
                    const unsigned long long m_ = __ballot(real);
                    if (real) {
                        const uint32_t at = cnt + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_, 0u));
                        if (at < (uint32_t)COO_CAP) { lpq[at] = row | (col << 8) | ((lab & ST_CZ) ? 0x10000u : 0u); lv[at] = v4[e]; }
                    }
                    cnt += (uint32_t)__popcll(m_);
                }
            }
            __syncthreads();
            if (cnt <= (uint32_t)COO_CAP) {
                cooRounds = (int)((cnt + 63u) >> 6);
#pragma unroll
                for (int e = 0; e < COO_E; ++e) {
                    const uint32_t at = (uint32_t)lane * (uint32_t)cooRounds + (uint32_t)e;   // (consecutive entries per lane, see above)
                    const bool have = e < cooRounds && at < cnt;
                    const uint32_t dummy = (uint32_t)L + (uint32_t)lane;                // inert: value 0 between two dummy elements
                    cpq[e] = have ? lpq[at] : (dummy | (dummy << 8) | 0x10000u);
                    cv[e] = have ? lv[at] : 0.0;
                }
            }
            __syncthreads();
        }
    }

    // ---- products of the vector x held in tk[] (elements >= 0), with xmax = max x and mp1 = 1 + the largest position with
    //      x > 0 (0: x is the zero vector):  split: (M x, C x) -> (Mn, Cn);  fused: (M + de C) x -> Mn (de >= 0; 0: M x alone)
    [[maybe_unused]] const double* pendRR = nullptr; [[maybe_unused]] bool pend = false;    // a posted reduction of (sum u', |u' - u|^2) waiting for its barrier
    double usum = 0.0, alpha = 1.0, unsum = 0.0, du2 = 0.0, xmaxT = 0.0;
    auto collect_pending = [&]() {
        if constexpr (NW != 1) {
            if (pend) { double q2[2]; block_collect<NW, 2>(q2, pendRR, tid); unsum = q2[0]; du2 = q2[1]; pend = false; }
        }
    };
    auto spmv = [&](double xmax, int mp1, const bool split, const double de_) {
        TMARK(3);
        if (!(xmax > 0.0) || mp1 <= 0) {                       // zero vector: zero products, nothing to publish
            if constexpr (NW != 1) { if (pend) { __syncthreads(); collect_pending(); } }
            FOR_K(k, p) { Mn[k] = 0.0; Cn[k] = 0.0; }
            ++n_pass;
            return;
        }
        const double de = (!split && de_ > 0.0) ? de_ : 0.0;    // what is added to a weight (wave-uniform)
        // scale: the largest term w x 2^s stays below 2^49: x_max 2^s in [2^48, 2^49) when the weights are those of M (<= 1),
        // and a further factor 2^(exponent(1 + de) + 1) >= 1 + de down when de is added to them
        int e_ = (int)((__double_as_longlong(xmax) >> 52) & 0x7ff) - 1023;
        int s_ = 48 - e_;
        if (de > 0.0) s_ -= (int)((__double_as_longlong(1.0 + de) >> 52) & 0x7ff) - 1023 + 1;
        s_ = s_ > 960 ? 960 : (s_ < -960 ? -960 : s_);
        const double sc = bits_f64((unsigned long long)(1023 + s_) << 52), inv = bits_f64((unsigned long long)(1023 - s_) << 52);
        // This wave's range of the stream and its first ST_D quads, requested BEFORE the vector is published: the matrix does
        // not depend on x, and a narrow pass is a dozen quads per wave — four or five dependent round trips to the L2 —, so the
        // first of them now runs under the publish, the barrier and its skew instead of behind them.  (Unconditional loads at
        // clamped indices, as in the loop below: the wait counters stay exact.  No quads at all: any valid address.)
        bool streamed = false;
        if constexpr (NW == 1) streamed = cooRounds >= 0;       // the matrix is in registers: pushes only
        const int Sx = (COOONLY || streamed) ? 0 : min(nsl, (mp1 + 63) >> 6);
        const uint32_t T = COOONLY ? 0u : CUMQ(Sx);
        const uint32_t qs = (uint32_t)(((unsigned long long)T * (unsigned)w) / NW), qe = (uint32_t)(((unsigned long long)T * (unsigned)(w + 1)) / NW);
        [[maybe_unused]] unsigned long long rc[ST_D]; [[maybe_unused]] dbl2_t rv0[ST_D], rv1[ST_D];
        if constexpr (!COOONLY) {
            const uint32_t qlast = (qe > qs ? qe : qs + 1u) - 1u;
            g_quad_cp cb0 = T ? cbase : (g_quad_cp)colsPool + lane;
            g_pair_cp vb0 = T ? vbase : (g_pair_cp)valsPool + lane;
#pragma unroll
            for (int t = 0; t < ST_D; ++t) {
                const uint32_t qq = min(qs + (uint32_t)t, qlast);
                rc[t] = cb0[(size_t)qq * 64];
                rv0[t] = vb0[(size_t)(2 * qq) * 64]; rv1[t] = vb0[(size_t)(2 * qq + 1) * 64];
            }
        }
        FOR_K(k, p) if (p < L) xg[p] = tk[k] * sc;
        __syncthreads();                                        // the scaled vector is published; accumulators are clean
        collect_pending();                                      // (the trial vector's sums, posted by finish_trial in front of this barrier)
        TMARK(6);
        if constexpr (NW == 1) {
            if (cooRounds >= 0) {
#pragma unroll
                for (int e = 0; e < COO_E; ++e) {
                    if (e < cooRounds) {
                        const uint32_t p_ = cpq[e] & 0xffu, q_ = (cpq[e] >> 8) & 0xffu;
                        const bool cz = HASCZ && (cpq[e] & 0x10000u);
                        const double xp_ = xl[p_], xq_ = xl[q_];
                        const double w_ = cz ? cv[e] : cv[e] + de;      // (split: de == 0, the weight of M)
                        if (xq_ != 0.0) {
                            __hip_atomic_fetch_add(aM + p_, (unsigned long long)__double_as_longlong(fma(w_, xq_, FX_MAGIC)) - FX_MAGIC_BITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (split && !cz) __hip_atomic_fetch_add(aC + p_, (unsigned long long)__double_as_longlong(xq_ + FX_MAGIC) - FX_MAGIC_BITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        if (xp_ != 0.0) {
                            __hip_atomic_fetch_add(aM + q_, (unsigned long long)__double_as_longlong(fma(w_, xp_, FX_MAGIC)) - FX_MAGIC_BITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (split && !cz) __hip_atomic_fetch_add(aC + q_, (unsigned long long)__double_as_longlong(xp_ + FX_MAGIC) - FX_MAGIC_BITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        __builtin_amdgcn_sched_barrier(0);      // (one round at a time: hoisting all six rounds' gathers costs a wave of occupancy)
                    }
                }
            }
        }
        // The stream itself, once per kind of pass (SPLIT a compile-time constant: the line search's fused passes carry no code
        // for the second sum).  A wave is alone with one other on its SIMD: nothing hides a latency for it, so the four gathers of
        // quad q + 1 are requested BEFORE quad q is worked on (its labels arrived with the ring), and the accumulators sit at fixed
        // distances LCAP behind the gathered vector — gather and push of a column share one address register.
        auto stream = [&](auto split_tag) {
            constexpr bool SPLIT = decltype(split_tag)::value;
            int s = 0;
            {   // largest s with cumQ[s] <= qs (skips empty slices)
                int lo_ = 0, hi_ = Sx;
                while (hi_ - lo_ > 1) { const int mid_ = (lo_ + hi_) >> 1; if (CUMQ(mid_) <= qs) lo_ = mid_; else hi_ = mid_; }
                s = lo_;
            }
            uint32_t nextB = CUMQ(s + 1);
            // ring of ST_D quads in flight per lane (filled above, in front of the barrier); loads are issued unconditionally
            // (clamped index) so that the wait counters stay exact
            unsigned long long smI = 0ull; [[maybe_unused]] unsigned long long scI = 0ull;   // pulled sums of this lane's row: sum of bits(MAGIC + term)
            uint32_t pieceQ = qs;                               // first quad of the current piece
            double xp = xl[s * 64 + lane];                      // this lane's row element (scaled); rows >= L read zeros
            double xpn = xl[(s + 1) * 64 + lane];               // ... and the next slice's, fetched ahead of the transition
            [[maybe_unused]] unsigned long long iCp = (unsigned long long)__double_as_longlong(xp + FX_MAGIC) - FX_MAGIC_BITS;
            // gathered elements of a quad: addresses (the accumulators of the same columns lie LCAP and 2 LCAP elements behind) and values
            l_vec_cp ga[4], gn[4]; double xa[4], xn[4];
#define UP_GATHER(C_, G_, X_)                                                                               \
            {                                                                                               \
                const uint32_t lo__ = (uint32_t)(C_), hi__ = (uint32_t)((C_) >> 32);                        \
                (G_)[0] = xl + (lo__ & ST_MASK); (G_)[1] = xl + ((lo__ >> 16) & ST_MASK);                   \
                (G_)[2] = xl + (hi__ & ST_MASK); (G_)[3] = xl + ((hi__ >> 16) & ST_MASK);                   \
                (X_)[0] = *(G_)[0]; (X_)[1] = *(G_)[1]; (X_)[2] = *(G_)[2]; (X_)[3] = *(G_)[3];             \
            }
#define UP_PUSH(G_, OFF_, V_) __hip_atomic_fetch_add((l_acc_p)(G_) + (OFF_), (V_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define UP_CONSUME(Q_, C_, V0_, V1_)                                                                        \
            {                                                                                               \
                [[maybe_unused]] const uint32_t clo = (uint32_t)(C_), chi = (uint32_t)((C_) >> 32);         \
                /* weights of this pass: v (split; fused with de == 0) or v + de, v alone where C_pq == 0 (inert entries  \
                   carry the flag when HASCZ: they keep their 0) */                                         \
                const double w0 = SPLIT ? (V0_).x : ((HASCZ && (clo & ST_CZ)) ? (V0_).x : (V0_).x + de);    \
                const double w1 = SPLIT ? (V0_).y : ((HASCZ && (clo & (ST_CZ << 16))) ? (V0_).y : (V0_).y + de); \
                const double w2 = SPLIT ? (V1_).x : ((HASCZ && (chi & ST_CZ)) ? (V1_).x : (V1_).x + de);    \
                const double w3 = SPLIT ? (V1_).y : ((HASCZ && (chi & (ST_CZ << 16))) ? (V1_).y : (V1_).y + de); \
                smI += (unsigned long long)__double_as_longlong(fma(w0, xa[0], FX_MAGIC));                  \
                smI += (unsigned long long)__double_as_longlong(fma(w1, xa[1], FX_MAGIC));                  \
                smI += (unsigned long long)__double_as_longlong(fma(w2, xa[2], FX_MAGIC));                  \
                smI += (unsigned long long)__double_as_longlong(fma(w3, xa[3], FX_MAGIC));                  \
                if constexpr (SPLIT) {                                                                      \
                    if (HASCZ) {                                                                            \
                        scI += (unsigned long long)__double_as_longlong(((clo & ST_CZ) ? 0.0 : xa[0]) + FX_MAGIC); \
                        scI += (unsigned long long)__double_as_longlong(((clo & (ST_CZ << 16)) ? 0.0 : xa[1]) + FX_MAGIC); \
                        scI += (unsigned long long)__double_as_longlong(((chi & ST_CZ) ? 0.0 : xa[2]) + FX_MAGIC); \
                        scI += (unsigned long long)__double_as_longlong(((chi & (ST_CZ << 16)) ? 0.0 : xa[3]) + FX_MAGIC); \
                    } else {          /* the only C-flagged entries are inert: they gather a zero */        \
                        scI += (unsigned long long)__double_as_longlong(xa[0] + FX_MAGIC);                  \
                        scI += (unsigned long long)__double_as_longlong(xa[1] + FX_MAGIC);                  \
                        scI += (unsigned long long)__double_as_longlong(xa[2] + FX_MAGIC);                  \
                        scI += (unsigned long long)__double_as_longlong(xa[3] + FX_MAGIC);                  \
                    }                                                                                       \
                }                                                                                           \
                if (xp != 0.0) {                      /* push this row's element to the columns */          \
                    UP_PUSH(ga[0], LCAP, (unsigned long long)__double_as_longlong(fma(w0, xp, FX_MAGIC)) - FX_MAGIC_BITS); \
                    UP_PUSH(ga[1], LCAP, (unsigned long long)__double_as_longlong(fma(w1, xp, FX_MAGIC)) - FX_MAGIC_BITS); \
                    UP_PUSH(ga[2], LCAP, (unsigned long long)__double_as_longlong(fma(w2, xp, FX_MAGIC)) - FX_MAGIC_BITS); \
                    UP_PUSH(ga[3], LCAP, (unsigned long long)__double_as_longlong(fma(w3, xp, FX_MAGIC)) - FX_MAGIC_BITS); \
                    if constexpr (SPLIT) {                                                                  \
                        if (!HASCZ || !(clo & ST_CZ)) UP_PUSH(ga[0], 2 * LCAP, iCp);                        \
                        if (!HASCZ || !(clo & (ST_CZ << 16))) UP_PUSH(ga[1], 2 * LCAP, iCp);                \
                        if (!HASCZ || !(chi & ST_CZ)) UP_PUSH(ga[2], 2 * LCAP, iCp);                        \
                        if (!HASCZ || !(chi & (ST_CZ << 16))) UP_PUSH(ga[3], 2 * LCAP, iCp);                \
                    }                                                                                       \
                }                                                                                           \
                if ((Q_) + 1 == nextB || (Q_) + 1 == qe) {            /* end of this slice's piece: flush the pulled sums */ \
                    const unsigned long long nterm = (unsigned long long)(((Q_) + 1 - pieceQ) * 4u) * FX_MAGIC_BITS; \
                    UP_PUSH(xl + (s * 64 + lane), LCAP, smI - nterm);                                       \
                    if constexpr (SPLIT) UP_PUSH(xl + (s * 64 + lane), 2 * LCAP, scI - nterm);              \
                    smI = 0ull; scI = 0ull; pieceQ = (Q_) + 1;                                              \
                    if ((Q_) + 1 < qe) {                                                                    \
                        const int s_old_ = s;                                                               \
                        do { ++s; nextB = CUMQ(s + 1); } while (nextB <= (Q_) + 1);                         \
                        xp = (s == s_old_ + 1) ? xpn : xl[s * 64 + lane];                                   \
                        xpn = xl[(s + 1) * 64 + lane];                                                      \
                        iCp = (unsigned long long)__double_as_longlong(xp + FX_MAGIC) - FX_MAGIC_BITS;      \
                    }                                                                                       \
                }                                                                                           \
            }
            UP_GATHER(rc[0], ga, xa)
            uint32_t q0 = qs;
            for (; q0 + ST_D <= qe; q0 += ST_D) {
#pragma unroll
                for (int t = 0; t < ST_D; ++t) {
                    const uint32_t q = q0 + t;
                    const unsigned long long c = rc[t];
                    const dbl2_t v0 = rv0[t], v1 = rv1[t];
                    const uint32_t qn = min(q + (uint32_t)ST_D, qe - 1u);
                    rc[t] = cbase[(size_t)qn * 64];
                    rv0[t] = vbase[(size_t)(2 * qn) * 64]; rv1[t] = vbase[(size_t)(2 * qn + 1) * 64];
                    UP_GATHER(rc[(t + 1) % ST_D], gn, xn)           // quad q + 1 (behind the last quad: a duplicate, unused)
                    UP_CONSUME(q, c, v0, v1)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { ga[e] = gn[e]; xa[e] = xn[e]; }
                }
            }
#pragma unroll
            for (int t = 0; t < ST_D; ++t) {                    // tail: fewer than ST_D quads, already in the ring
                const uint32_t q = q0 + t;
                if (q < qe) {
                    UP_GATHER(rc[(t + 1) % ST_D], gn, xn)
                    UP_CONSUME(q, rc[t], rv0[t], rv1[t])
#pragma unroll
                    for (int e = 0; e < 4; ++e) { ga[e] = gn[e]; xa[e] = xn[e]; }
                }
            }
#undef UP_CONSUME
#undef UP_PUSH
#undef UP_GATHER
        };
        if (!COOONLY && qs < qe) {
            if (split) stream(std::true_type{}); else stream(std::false_type{});
        }
        TMARK(Sx <= 2 ? 4 : 0);                                 // (timing build: the stream of narrow passes — at most two slices — apart)
        __syncthreads();                                        // every contribution has landed
        TMARK(1);
        FOR_K(k, p) {
            if (p < L) {
                Mn[k] = fx_decode(accM[p], inv); accM[p] = 0ull;            // clean for the next pass (published by its barrier)
                if (split) { Cn[k] = fx_decode(accC[p], inv); accC[p] = 0ull; } else Cn[k] = 0.0;
            } else { Mn[k] = 0.0; Cn[k] = 0.0; }
        }
        ++n_pass;
        TMARK(2);
    };

    // ---- the iteration as a state machine around ONE SpMV call site ------------------------------------
    enum { PH_RESCALE, PH_INIT, PH_TRIAL, PH_SPLIT };
    int phase = p_rescale ? PH_RESCALE : PH_INIT;
    int mp1T = 0;
    int i = 0, j = 0, kk = 0;

    auto normalize_u = [&]() {                                  // u /= |u|
        double r[1] = {0.0}, m0[1] = {0.0};
        FOR_K(k, p) r[0] += u[k] * u[k];
        block_red<NW, 1, 0>(r, m0, red, par, tid);
        const double nr = sqrt(r[0]);
        if (nr > 0.0) FOR_K(k, p) u[k] /= nr;                   // (three passes per problem: the exact division stays)
    };
    auto load_u_as_x = [&]() {                                  // x = u (initial passes): tk, its maximum and support bound
        double r0[1] = {0.0}, m2[2] = {0.0, 0.0};
        FOR_K(k, p) { tk[k] = u[k]; m2[0] = fmax(m2[0], u[k]); if (u[k] > 0.0) m2[1] = (double)(p + 1); }
        block_red<NW, 0, 2>(r0, m2, red, par, tid);             // NS == 0: r0 is not touched
        xmaxT = m2[0]; mp1T = (int)m2[1];
    };
    // gradient of the current u: ((s_p + d) u_p - d sum(u)) + ((M + d C) u)_p  (oracle: grad_and_F_fused)
    // trial vector u' = normalize(max(u + alpha g, 0)) into tk (+ its sums and support)
    // second half of a trial vector: tk holds max(u + alpha g, 0), r2 is its squared norm, m2 its maximum and 1 + its last
    // non-zero position -> tk normalised, its sums, its distance from u, its maximum and support bound
    auto finish_trial = [&](double r2, const double (&m2)[2]) {
        const double nr = sqrt(r2);
        double q[2] = {0.0, 0.0}, m0[1] = {0.0};                // sum u', |u'-u|^2
        FOR_K(k, p) {
            double t = tk[k];
            // (0 / nr == 0: an element outside the support skips the division — once the support has collapsed that is every
            //  element of seven of the eight waves, and an f64 division is ~40 instructions)
            if (nr > 0.0 && t != 0.0) { t /= nr; tk[k] = t; }
            q[0] += t;
            const double df = t - u[k]; q[1] += df * df;
        }
        TMARK(3);
        // sum u' and |u' - u|^2 are not looked at before the products of u' are back: their reduction rides on the barrier that
        // publishes u' (spmv collects it behind that barrier) instead of having one of its own — four workgroup barriers per
        // pass instead of five
        if constexpr (NW == 1) { block_red<NW, 2, 0>(q, m0, red, par, tid); unsum = q[0]; du2 = q[1]; }
        else { pendRR = block_post<NW, 2>(q, red, par, tid); pend = true; }
        TMARK(7);
        xmaxT = (nr > 0.0) ? m2[0] / nr : m2[0]; mp1T = (int)m2[1];
    };
    auto build_trial = [&]() {
        double r[1] = {0.0}, m2[2] = {0.0, 0.0};
        FOR_K(k, p) {
            const double up = u[k];
            const double g = ((sd[k] + d) * up - d * usum) + Wu[k];
            double t = up + alpha * g;
            t = (p < L && t > 0.0) ? t : 0.0;
            tk[k] = t; r[0] += t * t;
            m2[0] = fmax(m2[0], t);
            if (t > 0.0) m2[1] = (double)(p + 1);               // ascending p: the last one stays
        }
        TMARK(3);
        block_red<NW, 1, 2>(r, m2, red, par, tid);
        TMARK(6);
        finish_trial(r[0], m2);
    };
    auto objective = [&](const double (&uu)[KMAX], const double (&ww)[KMAX], double us) -> double {
        double r[1] = {0.0}, m0[1] = {0.0};
        FOR_K(k, p) {
            const double up = uu[k];
            const double g = ((sd[k] + d) * up - d * us) + ww[k];
            r[0] += up * g;
        }
        block_red<NW, 1, 0>(r, m0, red, par, tid);
        return r[0];
    };
    // mean of (M u)_p / Cbu_p over the active set, from the products (Mn, Cn) of the split pass over u just done
    auto d_ratio = [&](bool absval, double& acc, double& cnt) {
        double r2[2] = {0.0, 0.0}, m0[1] = {0.0};
        FOR_K(k, p) {
            const double up = u[k], Cbu = (usum - Cn[k]) - up;
            if (p < L && Cbu > p_eps && up > p_eps) { const double r_ = (Mn[k] + sd[k] * up) / Cbu; r2[0] += absval ? fabs(r_) : r_; r2[1] += 1.0; }
        }
        block_red<NW, 2, 0>(r2, m0, red, par, tid);
        acc = r2[0]; cnt = r2[1];
    };

    if (phase == PH_INIT) normalize_u();
    load_u_as_x();
    for (;;) {
        // RESCALE: M x alone (a fused pass with nothing added); INIT / SPLIT: both products; TRIAL: (M + d C) x
        spmv(xmaxT, mp1T, phase == PH_INIT || phase == PH_SPLIT, phase == PH_TRIAL ? d : 0.0);
        if (phase == PH_RESCALE) {                              // u = normalize(M u0 + diag u0)
            FOR_K(k, p) u[k] = (p < L) ? Mn[k] + sd[k] * u[k] : 0.0;
            normalize_u();
            load_u_as_x();
            phase = PH_INIT;
            continue;
        }
        if (phase == PH_INIT) {
            double r1[1] = {0.0}, m0[1] = {0.0};
            FOR_K(k, p) r1[0] += u[k];
            block_red<NW, 1, 0>(r1, m0, red, par, tid);
            usum = r1[0];
            double acc, cnt;
            d_ratio(false, acc, cnt);
            d = (cnt > 0.0) ? acc / cnt : 0.0;
            i = 0;
            if (i >= p_maxout) break;
        } else if (phase == PH_SPLIT) {                         // end of an inner loop: homotopy update of d from (M u, C u)
            double acc, cnt;
            d_ratio(true, acc, cnt);
            if (cnt > 0.0) d += acc / cnt; else break;
            ++i;
            if (i >= p_maxout) break;
        } else {                                                // PH_TRIAL: the fused product of the trial vector
            ++ls_trials;
            // (Forming the first half of the NEXT trial — max(u' + g(u'), 0), its norm, maximum and support bound — in the same
            //  reduction as this objective saves a workgroup barrier per accepted trial and was built in round 5: the four-value
            //  reduction and the discarded work of rejected trials cost more than the barrier, 0.99 against 0.96 ms per launch.)
            const double Fnew = objective(tk, Mn, unsum);
            const double deltaF = Fnew - F;
            if (deltaF < -p_eps && kk + 1 < p_maxls) {          // backtrack
                alpha *= p_beta; ++kk;
                build_trial();
                continue;
            }
            // accept: the trial vector and its product become the current ones
            const double du = sqrt(du2);
            F = Fnew; usum = unsum;
            FOR_K(k, p) { u[k] = tk[k]; Wu[k] = Mn[k]; }
            ++inner_iters; ++j;
            const bool stop = du < p_tol_u || fabs(deltaF) < p_tol_F;
            if (stop || j >= p_maxin) {                         // the d update needs M u and C u apart: one split pass over
                phase = PH_SPLIT;                               // the accepted vector (tk, xmaxT, mp1T are still its own)
                continue;
            }
        }
        if (phase != PH_TRIAL) {                                // a new outer iteration (INIT / SPLIT): the fused product at the new d
            FOR_K(k, p) Wu[k] = Mn[k] + Cn[k] * d;
            F = objective(u, Wu, usum); j = 0;
        }
        alpha = 1.0; kk = 0;
        build_trial();
        phase = PH_TRIAL;
    }
    if (i >= p_maxout) status |= ROMAN_ST_MAXITER;
    S.n_pass = n_pass; S.ls_trials = ls_trials; S.inner_iters = inner_iters;
    S.outer_iters = i; S.score = F; S.d_final = d;
#ifdef ROMAN_SOLVE_TIMING
    TMARK(3);
#endif
    // final u (unscaled) to LDS for the shared tail; scratch: the two accumulator arrays
    __syncthreads();
    FOR_K(k, p) if (p < L) xg[p] = u[k];
#ifdef ROMAN_SMALL_TIMING
    const unsigned long long tt0_ = __builtin_readcyclecounter();
    const unsigned long long tw1_ = wall_clock64();              // (100 MHz, the same on every compute unit: when did this problem's iteration end?)
#endif
    finish_one(D, b, pd, feats, assoc, plp, lpAsc, rowPosPool, nullptr, O, xg, reinterpret_cast<double*>(accM),
               reinterpret_cast<int32_t*>(accC), reinterpret_cast<int32_t*>(accC) + Lc, L, rb, lo, F, status, S, red, sint);
#ifdef ROMAN_SOLVE_TIMING
    if (tid == 0 && O.dbg) {                                    // slot 5: everything outside the phases (set-up in front of the first pass, the tail: selection, pose, outputs)
        unsigned long long sum_ = 0; for (int t = 0; t < 8; ++t) sum_ += tacc[t];
        tacc[5] = __builtin_readcyclecounter() - tentry_ - sum_; tcnt[5] = 1;
        unsigned long long* dg = O.dbg + (size_t)b * 16;
        for (int t = 0; t < 8; ++t) { dg[t] = tacc[t]; dg[8 + t] = tcnt[t]; }
    }
#endif
#ifdef ROMAN_SMALL_TIMING
    if (tid == 0 && ((b & 255) == 0 || b < 2 || (NW == 1 && n_pass >= 100)))
        printf("[solve_up<%d>] b=%d L=%d nnz=%llu passes %d tail (selection, pose, outputs) %llu cycles; wall clock (10 ns): entered %llu iteration done %llu left %llu\n", NW, b, L,
               (unsigned long long)st[b].nnzUpper, n_pass, __builtin_readcyclecounter() - tt0_, tw0_, tw1_, wall_clock64());
#endif
#undef FOR_K
#undef FOR_K_ALL
#undef CUMQ
}

// MAXL < STREAM_MAXL with NW = 1: the SMALL-problem instantiation — one wave per problem (no cross-wave barriers or
// reductions at all), 64-thread workgroups, many of them per compute unit: submaps of the reference's demo scale (20-40
// objects, ~60 live associations) would otherwise occupy a whole 8-wave workgroup — a whole compute unit, given the
// registers of the general instantiation — for ~100 entries of matrix.  [Llo, Lhi]: the live-set sizes this launch takes.
template <int NW, bool HASCZ, int MAXL>
__global__ void __launch_bounds__(NW * 64, NW == 1 ? 3 : 1) k_solve_up(DevParams D, int B, const ProbDesc* __restrict__ probs,
                                                      ProbState* __restrict__ st,
                                                      const double* __restrict__ feats, const int32_t* __restrict__ assoc,
                                                      const int32_t* __restrict__ plp, const int32_t* __restrict__ lpAsc,
                                                      const uint32_t* __restrict__ rowPos, const double* __restrict__ pld,
                                                      const uint32_t* __restrict__ sliceBase,
                                                      const uint16_t* __restrict__ cols, const double* __restrict__ vals,
                                                      const double* __restrict__ u0, SolveOut O,
                                                      int* __restrict__ queue, int Lc, int Llo, int Lhi, int R /* problems per claim: 1..64 */)
{
    // LDS: xg[Lc] f64 | accM[Lc] u64 | accC[Lc] u64 | red[red_doubles(NW)] | cumQ[ST_MAXSL + 2] u32 | sint[8]
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (Lc == MAXL + 64: solve_up addresses the accumulators at fixed distances from xg)
    double* xg = reinterpret_cast<double*>(smem);
    unsigned long long* accM = reinterpret_cast<unsigned long long*>(xg + Lc);
    unsigned long long* accC = accM + Lc;
    double* red = reinterpret_cast<double*>(accC + Lc);
    uint32_t* cumQ = reinterpret_cast<uint32_t*>(red + red_doubles(NW));
    int* sint = reinterpret_cast<int*>(cumQ + ST_MAXSL + 2);
    unsigned char* cooLds = reinterpret_cast<unsigned char*>(sint + 8);        // (one-wave instantiation only: COO_CAP * 12 bytes)
    for (;;) {
        // The first wave claims R consecutive problems at a time (R = 1 unless this launch expects to find nothing: a batch
        // of small problems passes through the general instantiation and vice versa) until the range holds one this launch
        // takes (stream layout, live-set size in [Llo, Lhi]): the others — the fallback solver's, skipped ones, the other
        // instantiation's — cost one atomic and two loads per range, no barrier.
        if (threadIdx.x < WAVE) {
            const int ln = threadIdx.x;
            int base_ = B; unsigned long long m_ = 0ull;
            for (;;) {
                int t_ = 0;
                if (ln == 0) t_ = atomicAdd(queue, R);
                base_ = __builtin_amdgcn_readfirstlane(t_);
                if (base_ >= B) break;
                const int b_ = base_ + ln;
                bool take = false;
                if (ln < R && b_ < B) { const int Lq = st[b_].L; take = st[b_].kind == 0 && Lq >= Llo && Lq <= Lhi; }
                m_ = __ballot(take);
                if (m_) break;
            }
            if (ln == 0) { sint[2] = base_; sint[3] = (int)(uint32_t)m_; sint[4] = (int)(uint32_t)(m_ >> 32); }
        }
        __syncthreads();
        const int base = uni(sint[2]);
        unsigned long long mask = ((unsigned long long)(uint32_t)uni(sint[4]) << 32) | (unsigned long long)(uint32_t)uni(sint[3]);
        __syncthreads();
        if (base >= B) break;
        while (mask) {
        const int b = base + __builtin_ctzll(mask);
        mask &= mask - 1ull;
        const ProbDesc pd = probs[b];
        solve_up<NW, HASCZ, MAXL>(D, b, pd, st, feats, assoc, plp, lpAsc, rowPos, pld, sliceBase, cols, vals, u0, O,
                                  xg, accM, accC, Lc, cumQ, red, sint, cooLds);
        __syncthreads();                                         // the next problem of the range reuses the LDS state
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_small: a problem of the reference's DEMO scale (submaps of 20-40 objects: ~60 live associations, ~110 stored pairs)
// from the live list to the pose in ONE kernel, one wave per problem, nothing but the result written to memory.  The general
// path spends eleven launches on such a problem (pair tests, mirror, prefix, sort, lists, geometry, scans, fill, solve ...):
// at 4096 problems per call every one of them costs 5-130 us for a few hundred bytes of work each.  Here lane = live row
// (two rows per lane: L <= SMALL_MAXL = 128):
//   pair tests   row k against every live column q, sequentially over q (both triangles: no transposition), the same
//                gate on the same table entries as k_count -> the row's candidate bits in registers;
//   positions    rank by (degree descending, row ascending): one sweep over the degrees in LDS — the order k_rowsort's
//                bitonic sort produces;
//   kept pairs   a candidate pair belongs to its endpoint of smaller position: listed in LDS, then evaluated 64 at a time
//                with k_fill_list's own value sequence (fill_value) and filter;
//   solve        the kept entries ARE the coordinate list the one-wave solver keeps in registers (solve_up, cooPre).
// Same candidates, same positions, same values, exact sums: the same bits as the general path.  A problem with more than
// SMALL_PAIR_CAP candidates or COO_CAP stored pairs is left to the general path (kind stays 0); a finished one becomes kind 3.
// ---------------------------------------------------------------------------------------------
constexpr int SMALL_PAIR_CAP = 2304;      // candidate pairs the LDS of the solver's three vectors can list (16 bits each)
// dynamic LDS of a k_small workgroup (the host launches with this): solver vectors | reduction scratch | slice table | sint | (16-byte
// alignment) | coordinate list | column data z / single score / objects / positions / degrees of up to SMALL_MAXL live associations
constexpr size_t small_lds_bytes()
{
    size_t o = (size_t)3 * 8 * (SMALL_MAXL + 64) + sizeof(double) * red_doubles(1) + sizeof(uint32_t) * (ST_MAXSL + 2) + sizeof(int) * 8;
    o = (o + 15) & ~(size_t)15;
    return o + (size_t)12 * COO_CAP + (size_t)SMALL_MAXL * (16 + 8 + 4 + 2 + 2);
}

__device__ __forceinline__ bool pair_gate_rt(const DevParams& D, int gm, double a, double bb, double dz)
{
    switch (gm) {
    case 1: return pair_gate<1>(D, a, bb, dz);
    case 2: return pair_gate<2>(D, a, bb, dz);
    case 3: return pair_gate<3>(D, a, bb, dz);
    default: return pair_gate<0>(D, a, bb, dz);
    }
}

template <bool FAST>
__global__ void __launch_bounds__(64, 3) k_small(DevParams D, int B, const ProbDesc* __restrict__ probs, ProbState* __restrict__ st,
                                              const double* __restrict__ feats, const int32_t* __restrict__ assoc,
                                              const double* __restrict__ tabPool,
                                              const int32_t* __restrict__ lp, const int32_t* __restrict__ li, const int32_t* __restrict__ lj,
                                              const double* __restrict__ ls, const double* __restrict__ ld,
                                              const double* __restrict__ lza, const double* __restrict__ lzb,
                                              int32_t* __restrict__ plp, double* __restrict__ pld, uint32_t* __restrict__ rowPos,
                                              const double* __restrict__ u0, SolveOut O, int* __restrict__ queue)
{
    // LDS: xg | accM | accC [Lc1 each] (before the solve: the candidate pair list) | red | cumQ | sint | coordinate list | cIJ | cZ | cS | posS | degS
    constexpr int Lc1 = SMALL_MAXL + 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* xg = reinterpret_cast<double*>(smem);
    unsigned long long* accM = reinterpret_cast<unsigned long long*>(xg + Lc1);
    unsigned long long* accC = accM + Lc1;
    double* red = reinterpret_cast<double*>(accC + Lc1);
    uint32_t* cumQ = reinterpret_cast<uint32_t*>(red + red_doubles(1));
    int* sint = reinterpret_cast<int*>(cumQ + ST_MAXSL + 2);
    unsigned char* cooLds = smem + (((size_t)(reinterpret_cast<unsigned char*>(sint + 8) - smem) + 15) & ~(size_t)15);   // 16-byte aligned (cZ behind it holds double2)
    uint32_t* lpq = reinterpret_cast<uint32_t*>(cooLds); double* lv = reinterpret_cast<double*>(cooLds + 4 * COO_CAP);
    double2* cZ = reinterpret_cast<double2*>(cooLds + 12 * COO_CAP);
    static_assert((12 * COO_CAP) % 16 == 0, "cZ alignment");
    double* cS = reinterpret_cast<double*>(cZ + SMALL_MAXL);
    uint32_t* cIJ = reinterpret_cast<uint32_t*>(cS + SMALL_MAXL);
    uint16_t* posS = reinterpret_cast<uint16_t*>(cIJ + SMALL_MAXL);
    uint16_t* degS = posS + SMALL_MAXL;
    uint16_t* pairs = reinterpret_cast<uint16_t*>(smem);       // (the solver's vectors are not in use yet)
    // (layout above == small_lds_bytes(): degS ends at cooLds + 12 COO_CAP + SMALL_MAXL (16 + 8 + 4 + 2 + 2))
    static_assert(SMALL_PAIR_CAP * 2 <= 3 * 8 * Lc1, "pair list fits the solver's vectors");
    const int lane = threadIdx.x;
    const int gm = D.gmode;
    for (;;) {
        {                                                       // one problem per claim: thousands of short problems balance over ~3000 resident waves
            int t_ = 0;
            if (lane == 0) t_ = atomicAdd(queue, 1);
            const int b = __builtin_amdgcn_readfirstlane(t_);
            if (b >= B) break;
            {
                const int Lq = uni_i(st[b].L);
                if (!(uni_i(st[b].kind) == 0 && Lq >= 1 && Lq <= SMALL_MAXL)) continue;
            }
            const ProbDesc pd = probs[b];
            const int L = uni_i(st[b].L);
            const int64_t lo = pd.liveOff;
            const double* TA = tabPool + pd.tabOff;
            const double* TB = TA + (int64_t)pd.n1 * pd.n1;
            __syncthreads();                                    // the previous problem is done with the LDS
#ifdef ROMAN_SMALL_TIMING
            unsigned long long ts_[8]; ts_[0] = __builtin_readcyclecounter();
#define SMARK(i_) ts_[i_] = __builtin_readcyclecounter()
#else
#define SMARK(i_) do { } while (0)
#endif
            // ---- rows ------------------------------------------------------------------------------------
            int ri[2], rj[2], rlp[2]; double rd[2], rza[2], rzb[2]; bool rv[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int k = r * 64 + lane;
                rv[r] = k < L;
                const int kk = rv[r] ? k : 0;
                ri[r] = li[lo + kk]; rj[r] = lj[lo + kk]; rlp[r] = lp[lo + kk]; rd[r] = ld[lo + kk];
                rza[r] = lza[lo + kk]; rzb[r] = lzb[lo + kk];
                if (rv[r]) { cIJ[k] = (uint32_t)ri[r] | ((uint32_t)rj[r] << 16); cZ[k] = make_double2(rza[r], rzb[r]); cS[k] = ls[lo + kk]; }
            }
            __syncthreads();
            SMARK(1);
            // ---- pair tests: row k against every live column ---------------------------------------------------
            unsigned long long m[2][2] = {{0ull, 0ull}, {0ull, 0ull}};
            const double* rowA[2] = {TA + (int64_t)ri[0] * pd.n1, TA + (int64_t)ri[1] * pd.n1};
            const double* rowB[2] = {TB + (int64_t)rj[0] * pd.n2, TB + (int64_t)rj[1] * pd.n2};
            const int nr = L > 64 ? 2 : 1;                      // row halves in use
#pragma unroll
            for (int wd = 0; wd < 2; ++wd) {
                const int q1 = min(L, (wd + 1) * 64);
                for (int q0 = wd * 64; q0 < q1; q0 += 4) {       // four columns at a time: their table gathers (global memory) in flight together
                    uint32_t pk[4]; double2 zz[4]; double a[2][4], bb[2][4];
#pragma unroll
                    for (int x = 0; x < 4; ++x) { const int q = min(q0 + x, q1 - 1); pk[x] = cIJ[q]; zz[x] = cZ[q]; }
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int r = 0; r < 2; ++r)
                            if (r < nr) { a[r][x] = rowA[r][pk[x] & 0xffffu]; bb[r][x] = rowB[r][pk[x] >> 16]; }
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        if (q0 + x < q1) {
#pragma unroll
                            for (int r = 0; r < 2; ++r) {
                                if (r < nr) {
                                    const double dz = gm ? fabs((rza[r] - zz[x].x) - (rzb[r] - zz[x].y)) : 0.0;
                                    const bool is = pair_gate_rt(D, gm, a[r][x], bb[r][x], dz);
                                    m[r][wd] |= (unsigned long long)(is ? 1u : 0u) << ((q0 + x) & 63);
                                }
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) if (!rv[r]) { m[r][0] = 0ull; m[r][1] = 0ull; }
            SMARK(2);
            // ---- positions: rank by (degree descending, row ascending) -----------------------------------------
            int dg[2], pos[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) { dg[r] = __popcll(m[r][0]) + __popcll(m[r][1]); if (rv[r]) degS[r * 64 + lane] = (uint16_t)dg[r]; }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int rank = 0;
                const int k = r * 64 + lane;
                if (r < nr) for (int k2 = 0; k2 < L; ++k2) { const int d2 = (int)degS[k2]; rank += (d2 > dg[r] || (d2 == dg[r] && k2 < k)) ? 1 : 0; }
                pos[r] = rank;
                if (rv[r]) { posS[k] = (uint16_t)rank; rowPos[lo + k] = (uint32_t)rank; plp[lo + rank] = rlp[r]; pld[lo + rank] = rd[r]; }
            }
            __syncthreads();
            SMARK(3);
            // ---- the candidates a row KEEPS: those whose position is larger than its own ---------------------------
            uint32_t cnt[2] = {0u, 0u};
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int wd = 0; wd < 2; ++wd) {
                    unsigned long long x = m[r][wd], keep = 0ull;
                    while (x) {
                        const int bit = __builtin_ctzll(x);
                        x &= x - 1ull;
                        if ((int)posS[wd * 64 + bit] > pos[r]) { keep |= 1ull << bit; ++cnt[r]; }
                    }
                    m[r][wd] = keep;
                }
            const uint32_t inc0 = wave_incl_scan(cnt[0]), tot0 = (uint32_t)__builtin_amdgcn_readlane((int)inc0, 63);
            const uint32_t inc1 = wave_incl_scan(cnt[1]), tot1 = (uint32_t)__builtin_amdgcn_readlane((int)inc1, 63);
            const uint32_t cand = tot0 + tot1;
            if (cand > (uint32_t)SMALL_PAIR_CAP) continue;       // too many candidates for the list: the general path takes the problem
            uint32_t off[2] = {inc0 - cnt[0], tot0 + inc1 - cnt[1]};
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int wd = 0; wd < 2; ++wd) {
                    unsigned long long x = m[r][wd];
                    while (x) {
                        const int bit = __builtin_ctzll(x);
                        x &= x - 1ull;
                        pairs[off[r]++] = (uint16_t)((r * 64 + lane) | ((wd * 64 + bit) << 8));
                    }
                }
            __syncthreads();
            SMARK(4);
            // ---- values of the kept candidates, 64 at a time; entries above affinityeps form the coordinate list -------------
            uint32_t nk = 0;
            for (uint32_t c0 = 0; c0 < cand; c0 += 64u) {
                const uint32_t idx = c0 + (uint32_t)lane;
                const bool have = idx < cand;
                const uint32_t pr = pairs[have ? idx : 0u];
                const int k = (int)(pr & 0xffu), q = (int)(pr >> 8);
                const uint32_t pkk = cIJ[k], pkq = cIJ[q];
                const double a = TA[(int64_t)(pkk & 0xffffu) * pd.n1 + (pkq & 0xffffu)], bb = TB[(int64_t)(pkk >> 16) * pd.n2 + (pkq >> 16)];
                const double2 zk = cZ[k], zq = cZ[q];
                const double sk = cS[k], sq = cS[q];
                double v;
                if (D.gravity) v = fill_value<true, FAST>(D, a, bb, zk.x - zq.x, zk.y - zq.y, sk * sq, sk, sq);
                else v = fill_value<false, FAST>(D, a, bb, 0.0, 0.0, sk * sq, sk, sq);
                const bool keep = have && v > D.p.affinityeps;
                const unsigned long long km = __ballot(keep);
                if (keep) {
                    const uint32_t at = nk + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
                    if (at < (uint32_t)COO_CAP) { lpq[at] = (uint32_t)posS[k] | ((uint32_t)posS[q] << 8); lv[at] = v; }
                }
                nk += (uint32_t)__popcll(km);
            }
            if (nk > (uint32_t)COO_CAP) continue;                // more stored pairs than the registers hold: the general path
            if (lane == 0) st[b].nnzUpper = (unsigned long long)nk;
            __syncthreads();                                    // the pair list is spent: its LDS becomes the solver's vectors
            SMARK(5);
            solve_up<1, false, SMALL_MAXL, true>(D, b, pd, st, feats, assoc, plp, lp, rowPos, pld, nullptr, nullptr, nullptr, u0, O,
                                           xg, accM, accC, Lc1, cumQ, red, sint, cooLds, (int)nk, (int)lo);
            if (lane == 0) st[b].kind = 3;                      // done: the general kernels pass it by
#ifdef ROMAN_SMALL_TIMING
            SMARK(6);
            if (lane == 0 && ((b & 255) == 0 || B <= 4)) printf("[k_small] b=%d L=%d cand=%u nnz=%u cycles: rows %llu tests %llu ranks %llu keep %llu values %llu solve+tail %llu\n", b, L, cand, nk,
                                                                ts_[1] - ts_[0], ts_[2] - ts_[1], ts_[3] - ts_[2], ts_[4] - ts_[3], ts_[5] - ts_[4], ts_[6] - ts_[5]);
#endif
#undef SMARK
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_solve_wide: the solver for FEW, LARGE problems of the fallback kind (symmetric sorted SELL-64): every compute unit
// works on ONE problem at a time.  (`method='gravity'` / `'clipper'` at n = m = 200, or the ROMAN_SINGLE_DIAG_KEEP
// reading: L = 40 000 live associations, 0.5 GB of matrix; one workgroup would stream that at a few GB/s.)
//
//  * One persistent launch, one 512-thread workgroup per compute unit (cooperative launch: all resident).
//  * The matrix is ONE flat stream of T "steps" (a step = one quad of the 64 lanes of a slice: 4 column words and 4
//    values per lane, three 16-byte loads), cut into chunks that are dealt round-robin to the waves of the grid (chunk c
//    to wave c mod NWG: at any moment the grid reads one contiguous window of the matrix; every wave takes the same
//    number of chunks) whatever slices they belong to; a wave keeps two blocks of WIDE_U quads in flight and leaves the partial row sums of every slice piece it
//    covered in a partials buffer (piece id = chunk + slice).  The rows' owners add the pieces of their slice in
//    ascending order — a fixed order, no atomics.  (The round-2 solver gave a whole slice to one wave: 625 waves of
//    4096 busy, each walking ~1000 dependent steps: 0.5 ms per pass of pure latency.)
//  * Vector elements live in REGISTERS: thread (wave g, lane l) owns positions (g + k NWG) * 64 + l — the rows of the slices
//    whose partials it adds.  Only the vector being multiplied is in memory (live order, gathered by column index).
//  * The trial vector is published UNNORMALISED: t = max(u + alpha grad, 0) goes out together with the partials of
//    sum t^2 and sum t under ONE grid barrier; M t, C t come back and are scaled by 1 / |t| in registers
//    (M (t / |t|) = (M t) / |t| up to rounding).  A line-search trial costs TWO grid barriers: behind the stream, and one
//    that carries the trial's objective together with the sums of BOTH vectors that can come next (the backtracked
//    trial and the first trial from the accepted vector are published speculatively before the objective is known).
//  * Grid barrier: one monotone counter; everything other workgroups read is stored write-through (`sc1`), so an
//    arrival is: every wave drains its stores, workgroup barrier, one relaxed atomic add; departure: relaxed poll,
//    ONE agent-scope acquire, workgroup barrier (MI355X_MICROARCH.md "barrier-counter": 7 us against 26 us for
//    cooperative_groups' grid.sync()).  Grid sums ride on it: workgroup partials into a ping-pong slot array before the
//    arrival, every workgroup adds the slots in one fixed order afterwards.  Every spin is bounded (4 s): on a timeout the
//    kernel gives up and reports ROMAN_ST_INTERNAL instead of hanging the device.
//  * Column compaction (round 4): the team keeps books on the published support bit maps and, when the support has left half
//    of the columns in use, rewrites the matrix without them into a mirror of the pools and streams that copy (see `stream`).
//  Mirrors oracle_solve() like solve_one; the sums are plain doubles in a fixed (different) order.
// ---------------------------------------------------------------------------------------------
constexpr int WIDE_NT = 512;             // threads per workgroup (one workgroup per compute unit; 8 waves: 256 registers each)
constexpr int WIDE_NW = WIDE_NT / 64;
constexpr int WIDE_KW = 2;               // vector elements a thread can own: L <= WIDE_KW * 64 * (waves of the grid)
constexpr int WIDE_NRED = 10;            // doubles per workgroup slot of a grid reduction
constexpr int WIDE_MAXBLK = 8;           // column blocks of the half copy (pull + push passes) at most
constexpr int WIDE_U = 3;                // quads (of 4 entries per lane) per block of the stream; two blocks in flight per wave
constexpr int WIDE_MAXCH = 8;            // chunks of the flat stream a wave takes per pass at most

// dynamic LDS of k_solve_wide in front of the gathered vector's leading part: three bit maps of bmWords 64-bit words and the
// cumulative slice widths (bmWords + 2 32-bit words), rounded up to 16 bytes (host and kernel use this one function)
__host__ __device__ constexpr size_t wide_fixed_lds(int bmWords) { return ((size_t)3 * 8 * (size_t)bmWords + 4 * ((size_t)bmWords + 2) + 15) & ~(size_t)15; }

struct WideShared {
    double wred[2][WIDE_NW][WIDE_NRED];  // wave partials of a reduction (ping-pong)
    double bc[2][WIDE_NRED];             // reduced values for the whole workgroup (ping-pong)
    double red[72];                      // finish_one scratch
    int sint[4];
    int abort_;
    int sS[WIDE_NT / 64][8];             // per wave: first slice of each of its chunks (-1: no such chunk)
    // the half copy (pull + push passes): per column block its stream's steps, steps per chunk, first piece id, first step in the
    // mirror pools, the team's workgroups that stream it (count, first rank)
    uint32_t upT[WIDE_MAXBLK], upCS[WIDE_MAXBLK], upPB[WIDE_MAXBLK], upSB[WIDE_MAXBLK];
    int upG[WIDE_MAXBLK], upCU[WIDE_MAXBLK];
    int upI[4];                          // column blocks, columns per block, my block, steps of the copy (read where needed: not kept in registers)
    double upFx;                         // 2^-s of the pass on the copy
};

// write-through store of a value other workgroups will read (global_store ... sc1: no release fence needed later)
__device__ __forceinline__ void st_pub(double* p, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid barrier, XCD-hierarchical (MI355X_MICROARCH.md "barrier-xcd": 4-5 us against 7+ for one flat counter and 26 for
// cooperative_groups' grid.sync()): a workgroup arrives at the counter of the XCD it runs on; the last arriver of an XCD
// arrives at the top counter, waits for the other XCDs' leaders and then releases its own XCD through a generation word that
// the others poll — 32 + 8 serialised atomics instead of 256, and nobody polls a line that arrivals are still hitting.
// Which XCD a workgroup is on is read from the hardware (HW_REG_XCC_ID), how many workgroups each XCD holds is counted at
// kernel start (wide_census): nothing is assumed about placement.  Words of `bar` (zeroed before every launch), one 128-byte
// line each: [0] abort flag, [1+x] arrivals of XCD x, [9] top arrivals, [10+x] generation of XCD x, [18] census (8 words),
// [19] flat counter of the census barrier.  RELEASE: plain stores issued before the barrier must be visible behind it as well.
// Every spin is bounded (4 s): on a timeout the abort flag goes up and every workgroup leaves.
// TEAM mode (several fallback problems in a batch): the workgroups of an XCD — or of a half / a quarter of it (`sub` teams per
// XCD) — form a team that solves its own problem; a team barrier is ONE level (the team's counter, released by the last
// arriver through the team's generation word) and the teams never meet after the census.  Further lines of `bar`: [20] the
// problem queue, [21] number of fallback problems (written by k_skipped), [24 + t] arrivals of team t, [56 + t] generation
// of team t (t < 32).
constexpr int WIDE_MAX_TEAMS = 32;
constexpr int WIDE_BAR_WORDS = (56 + WIDE_MAX_TEAMS) * 32;
struct WideBar { unsigned* bar; unsigned epoch; int G; int xcc; unsigned nX; unsigned nActive; unsigned long long budget /* wall-clock ticks a spin may last */;
                 int teamMode; int tG /* workgroups of my team */; int tRank /* my rank in it */; int team; };

__device__ __forceinline__ bool wide_spin(const unsigned* word, unsigned target, unsigned* bar, unsigned long long budget)
{
    const unsigned long long t0 = wall_clock64();
    unsigned n = 0;
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        // (budget 0 — the test hook ROMAN_WIDE_SPIN_MS=0 — makes the very first unsuccessful poll a timeout)
        if (((++n & 255u) == 0u || budget == 0ull) && (wall_clock64() - t0 > budget || __hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            __hip_atomic_store(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
    }
    return true;
}

template <bool RELEASE>
__device__ __forceinline__ bool wide_sync(WideShared& sh, WideBar& wb, int ltid)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // every wave: its stores have left the compute unit
    __syncthreads();
    ++wb.epoch;
    if (ltid == 0) {
        if (RELEASE) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        unsigned* bar = wb.bar;
        bool ok = true;
        if (wb.teamMode) {                                      // one level: the team's counter, the last arriver releases the team
            const unsigned old = __hip_atomic_fetch_add(bar + 32 * (24 + wb.team), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old + 1u == wb.epoch * (unsigned)wb.tG) __hip_atomic_store(bar + 32 * (56 + wb.team), wb.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else ok = wide_spin(bar + 32 * (56 + wb.team), wb.epoch, bar, wb.budget);
            if (!ok) sh.abort_ = 1;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        } else {
        const unsigned old = __hip_atomic_fetch_add(bar + 32 * (1 + wb.xcc), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == wb.epoch * wb.nX) {                     // the last workgroup of this XCD: on to the top level
            __hip_atomic_fetch_add(bar + 32 * 9, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = wide_spin(bar + 32 * 9, wb.epoch * wb.nActive, bar, wb.budget);
            // (a leader that gave up does NOT release its XCD: the abort flag is up, its peers see it within 256 polls and
            //  leave from this barrier instead of walking into the next one)
            if (ok) __hip_atomic_store(bar + 32 * (10 + wb.xcc), wb.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            ok = wide_spin(bar + 32 * (10 + wb.xcc), wb.epoch, bar, wb.budget);
        }
        if (!ok) sh.abort_ = 1;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // this compute unit's L1 holds nothing older than the barrier
        }
    }
    __syncthreads();
    return sh.abort_ == 0;
}

// Once per launch: which XCD am I on, how many workgroups does each XCD hold (one flat-counter barrier).
__device__ __forceinline__ bool wide_census(WideShared& sh, WideBar& wb, int ltid)
{
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    wb.xcc = (int)(x & 7u);
    if (ltid == 0) {
        unsigned* bar = wb.bar;
        sh.sint[2] = (int)__hip_atomic_fetch_add(bar + 32 * 18 + wb.xcc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // my rank among the XCD's workgroups
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(bar + 32 * 19, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool ok = wide_spin(bar + 32 * 19, (unsigned)wb.G, bar, wb.budget);
        unsigned act = 0;
        for (int t = 0; t < 8; ++t) {
            const unsigned c_ = __hip_atomic_load(bar + 32 * 18 + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            act += c_ ? 1u : 0u;
            if (t == wb.xcc) sh.sint[0] = (int)c_;
        }
        sh.sint[1] = (int)act;
        if (!ok) sh.abort_ = 1;
    }
    __syncthreads();
    wb.nX = (unsigned)sh.sint[0]; wb.nActive = (unsigned)sh.sint[1];
    const int rankX = sh.sint[2];
    __syncthreads();
    if (wb.teamMode) {                                          // `teamMode` sub-teams per XCD: ranks [first(s), first(s + 1)), first(s) = ceil(s nX / sub)
        const int sub = wb.teamMode, nX = (int)wb.nX;
        const int sidx = min(sub - 1, (rankX * sub) / max(nX, 1));
        const int f0 = (sidx * nX + sub - 1) / sub, f1 = ((sidx + 1) * nX + sub - 1) / sub;
        // (rank r belongs to sub-team floor(r sub / nX) — first(s) is the smallest r with r sub >= s nX)
        wb.tG = f1 - f0; wb.tRank = rankX - f0; wb.team = wb.xcc * sub + sidx;
    } else { wb.tG = wb.G; wb.tRank = (int)blockIdx.x; wb.team = 0; }
    return sh.abort_ == 0;
}

// Grid barrier carrying N values: v[i] <- sum (i < N - NM) or maximum (the last NM, non-negative values) over every thread
// of the grid, identical in all of them (fixed order: lanes by butterfly, waves ascending, workgroups lane-strided then
// butterfly).  N == 0: the barrier alone.
template <int N, int NM = 0>
__device__ __forceinline__ bool wide_reduce(double (&v)[N > 0 ? N : 1], WideShared& sh, double* slots, WideBar& wb, int ltid)
{
    static_assert(N <= WIDE_NRED && NM <= N, "slot width");
    const int lane = ltid & 63, w = ltid >> 6, par = (int)(wb.epoch & 1u);
    const int G = wb.tG;                                        // the team's workgroups (whole-device mode: the grid)
    slots += (size_t)wb.team * 2 * (size_t)wb.G * WIDE_NRED;    // a team's own ping-pong slot array
    if (N > 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double x = v[i];
            if (i < N - NM) { for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off); }
            else { for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off)); }
            if (lane == 0) sh.wred[par][w][i] = x;
        }
        __syncthreads();
        if (ltid < N) {
            double t = 0.0;
            if (ltid < N - NM) { for (int ww = 0; ww < WIDE_NW; ++ww) t += sh.wred[par][ww][ltid]; }
            else { for (int ww = 0; ww < WIDE_NW; ++ww) t = fmax(t, sh.wred[par][ww][ltid]); }
            st_pub(slots + ((size_t)par * G + wb.tRank) * WIDE_NRED + ltid, t);
        }
    }
    if (!wide_sync<false>(sh, wb, ltid)) return false;
    if (N > 0) {
        if (w == 0) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double a = 0.0;
                if (i < N - NM) {
                    for (int g = lane; g < G; g += WAVE) a += slots[((size_t)par * G + g) * WIDE_NRED + i];
                    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
                } else {
                    for (int g = lane; g < G; g += WAVE) a = fmax(a, slots[((size_t)par * G + g) * WIDE_NRED + i]);
                    for (int off = 32; off > 0; off >>= 1) a = fmax(a, __shfl_xor(a, off));
                }
                if (lane == 0) sh.bc[par][i] = a;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = sh.bc[par][i];
    }
    return true;
}

template <typename IdxT, bool HALF /* the instantiation that can run pull + push passes over a half copy of the matrix (build_upper; 16-bit labels) */>
__global__ void __launch_bounds__(WIDE_NT) k_solve_wide(DevParams D, int B, const ProbDesc* __restrict__ probs,
                                                        ProbState* __restrict__ st,
                                                        const double* __restrict__ feats, const int32_t* __restrict__ assoc,
                                                        const int32_t* __restrict__ lp, const double* __restrict__ ld,
                                                        const uint32_t* __restrict__ permPool, const uint32_t* __restrict__ rowPosPool,
                                                        const uint32_t* __restrict__ sliceBasePool,
                                                        const IdxT* __restrict__ colsPool, const double* __restrict__ valsPool,
                                                        double* __restrict__ vU /* final u by position */,
                                                        double* __restrict__ vXa, double* __restrict__ vXb /* published vectors, by position */,
                                                        double* __restrict__ vS0, double* __restrict__ vS1, double* __restrict__ vS2 /* scratch of the shared tail */,
                                                        int32_t* __restrict__ plp /* position -> association index (written here) */,
                                                        const double* __restrict__ u0, SolveOut O,
                                                        double* __restrict__ part /* [(chunks + slices)][64][2] */,
                                                        double* __restrict__ slots /* [2][G][WIDE_NRED] */, unsigned* __restrict__ bar,
                                                        unsigned long long* __restrict__ bmPool /* [2][bmWords]: support bit maps of the two published vectors */,
                                                        int bmWords /* 64-bit words of one bit map (and of its LDS copy) */,
                                                        int xcap /* doubles of dynamic LDS behind the bit map: the gathered vector's leading part */,
                                                        unsigned long long spinTicks /* wall-clock ticks a barrier wait may last (host: 4 s at the device's wall-clock rate) */,
                                                        int teams /* 0: the whole device on one problem at a time; s >= 1: s teams per XCD, a problem each */,
                                                        const int32_t* __restrict__ fbList /* the batch's fallback problems (k_skipped) */,
                                                        long long partStride /* doubles of `part` a team owns */,
                                                        IdxT* colsC, double* valsC /* (no __restrict__: a compacted copy is compacted again in place) mirror of the matrix pools: the column-compacted copy (same offsets) */,
                                                        int ccfg /* column compaction: bits 0-7 compactions allowed per problem (0: off), 8-15 threshold (x / 256 of the columns in use), 16-23 passes per window */,
                                                        int ucfg /* bit 0: pull + push passes over a half copy of the matrix — every pair stored once — (16-bit labels only) while no compacted copy exists */,
                                                        unsigned long long* __restrict__ yPart /* [team][ySlots][2][ycap]: a workgroup's pushed fixed-point sums of its column block (M x, C x) */,
                                                        int ySlots /* workgroups of a team the host sized yPart for */, int ycap /* columns of a block at most (multiple of 64, 3 ycap <= xcap) */,
                                                        uint32_t* __restrict__ upMeta /* [team][WIDE_MAXBLK][bmWords + 1]: slice widths (steps) of the half copy per column block */)
{
    __shared__ WideShared sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char wide_smem[];
    unsigned long long* bml = reinterpret_cast<unsigned long long*>(wide_smem);      // support bit map of the vector being multiplied
    unsigned long long* bmC = bml + bmWords;                                         // columns of the compacted copy in use
    unsigned long long* bmA = bmC + bmWords;                                         // union of the supports multiplied in the current window
    uint32_t* cw = reinterpret_cast<uint32_t*>(bmA + bmWords);                       // cumulative slice widths (steps) of the stream in use: bmWords + 1 (+ 1 pad)
    double* xl = reinterpret_cast<double*>(wide_smem + wide_fixed_lds(bmWords));     // the multiplied vector's leading xcap elements (16-byte aligned)
    const roman_params_t& P = D.p;
    const int ltid = threadIdx.x, lane = ltid & 63, w = uni_i(ltid >> 6);
    if (ltid == 0) { sh.abort_ = 0; sh.upI[3] = 0; }
    __syncthreads();
    WideBar wb{bar, 0u, (int)gridDim.x, 0, 1u, 1u, spinTicks, teams, (int)gridDim.x, (int)blockIdx.x, 0};
    // (a problem this launch does not finish keeps the record k_skipped pre-wrote for it: ROMAN_ST_INTERNAL, no associations,
    //  NaN pose — whatever exit a workgroup takes after a bounded wait expired, nothing stale is left behind)
    if (!wide_census(sh, wb, ltid)) return;
    const int G = wb.tG, NWG = G * WIDE_NW;                      // my team (whole-device mode: the grid)
    const int gw = w * G + wb.tRank;                            // wave id in the team: consecutive ids on different compute units
    part += (size_t)wb.team * (size_t)partStride;
    bmPool += (size_t)wb.team * 3 * (size_t)bmWords;            // two bit maps + the new slice widths of a compaction
    uint32_t* wNew = reinterpret_cast<uint32_t*>(bmPool + 2 * (size_t)bmWords);
    const int cmax = ccfg & 0xff, cthr = (ccfg >> 8) & 0xff, cwin = max(1, (ccfg >> 16) & 0xff);
    const int nFb = (int)__hip_atomic_load(bar + 32 * 21, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int jq = 0; ; ++jq) {
        int b;
        if (teams) {                                            // the team's first workgroup claims the next problem; a barrier carries it to the others
            double claim[1] = {0.0};
            if (wb.tRank == 0) {
                if (ltid == 0) { const unsigned j_ = __hip_atomic_fetch_add(bar + 32 * 20, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); sh.sint[3] = j_ < (unsigned)nFb ? fbList[j_] + 1 : 0; }
                __syncthreads();
                claim[0] = (double)sh.sint[3];
                __syncthreads();
            }
            if (!wide_reduce<1, 1>(claim, sh, slots, wb, ltid)) return;
            b = (int)claim[0] - 1;
            if (b < 0) break;
        } else {
            if (jq >= nFb) break;
            b = fbList[jq];
        }
        b = uni_i(b);
        // beyond this team's registers or its share of the partials buffer (the host sizes teams so that this does not happen):
        // the problem keeps its pre-written ROMAN_ST_INTERNAL record
        if ((int64_t)WIDE_KW * NWG * 64 < (int64_t)st[b].L ||
            ((int64_t)NWG * WIDE_MAXCH + (((int64_t)st[b].L + 63) >> 6) + 4) * 128 > (int64_t)partStride) continue;
        const ProbDesc pd = probs[b];
        const int L = uni_i(st[b].L), rb = uni_i(st[b].rowBase);
        const int64_t lo = pd.liveOff;
        const int nsl = (L + 63) >> 6;
        const uint32_t Tfull = st[b].nnzCap >> 8;               // steps of the flat stream (a step = one quad of the 64 lanes of a slice: 256 entries)
        const uint32_t* perm = permPool + lo; const uint32_t* sbase = sliceBasePool + lo;
        const IdxT* cols = colsPool + st[b].nnzOff; const double* vals = valsPool + st[b].nnzOff;
        IdxT* colsK = colsC + st[b].nnzOff; double* valsK = valsC + st[b].nnzOff;   // the compacted copy: same slice bases, fewer steps per slice
        double* xva = vXa + rb; double* xvb = vXb + rb;
        unsigned long long* bma = bmPool; unsigned long long* bmb = bmPool + bmWords;
        const int kw = min(WIDE_KW, (nsl + NWG - 1) / NWG);     // element rounds in use (the host guarantees L <= WIDE_KW * NWG * 64)
#define CUMW(s_) (cw[(s_)])
#define MEMW(s_) (sbase[(s_)] >> 8)                              /* first step of slice s_ in memory (both copies) */
#define FORK(k_) _Pragma("unroll") for (int k_ = 0; k_ < WIDE_KW; ++k_) if (k_ < kw)
        // The stream in use: the full matrix (cw = the layout's own slice bases) or its column-compacted copy (fewer steps per
        // slice, the slices at their old places).  Chunks of CS steps, dealt round-robin to the waves (chunk c to wave c % NWG):
        // at any moment the waves of the grid read one contiguous window of the matrix.  Every wave takes the same number
        // m <= WIDE_MAXCH of chunks (the last round may be short): about 96 steps per chunk (chunk_steps), more when the matrix is larger.
        uint32_t T = Tfull, CS = 1u, nCh = 0u;
        int cmode = 0 /* stream in use: 0 full, 1 the column-compacted copy, 2 my column block of the half copy (pull + push) */, ncomp = 0, winPass = 0, winOut = 0; bool haveCopy = false;
        int cNWG = NWG, cgw = gw;                              // the waves the stream in use is dealt to and my id among them (half copy: the workgroups of my column block)
        // the half copy: column blocks, their width, my block, its workgroups / my rank among them, its first column, the fixed-point scale of the pass
        bool upOn = false;                                      // (everything else about the copy lives in sh.up*: read where needed, no registers across the passes)
        uint32_t copyCols = 0u, Tcopy = 0u;                     // compaction state (identical in every workgroup of the team)
        uint32_t pcf[WIDE_KW], pcn[WIDE_KW];
        static_assert(WIDE_MAXCH <= 8, "sS capacity");
        auto chunk_steps = [&](uint32_t T_, uint32_t nwg_) -> uint32_t {   // steps per chunk of a stream of T_ steps dealt to nwg_ waves
            // (about 96 steps per chunk: one or two long chunks per wave — round 3 had settled on 16 steps, up to eight chunks per wave; measured
            //  again in round 6, one / two / four / auto chunks per wave: 64 x L = 10 000 37.8 / 37.9 / 38.4 / 40.0 ms of solve, on the half copy
            //  35.5 / 35.1 / 37.4 / 37.0; n = m = 200 21.8 / 22.3 / 22.8 / 22.4 — fewer pieces per slice for the owners to collect)
            const uint32_t mch = max(1u, min((uint32_t)WIDE_MAXCH, (T_ + nwg_ * 96u - 1u) / (nwg_ * 96u)));
            return max(1u, (T_ + nwg_ * mch - 1u) / (nwg_ * mch));
        };
        auto geometry = [&]() {                                 // (cw, T, cNWG and cgw are set; every thread of the workgroup calls this)
            CS = chunk_steps(T, (uint32_t)cNWG);
            nCh = (T + CS - 1u) / CS;                            // <= cNWG * WIDE_MAXCH
            __syncthreads();                                    // (the previous stream is done with sS; cw is complete)
            if (lane < WIDE_MAXCH) {                            // lane j: first slice of this wave's chunk j (-1: no such chunk)
                const uint32_t c = (uint32_t)cgw + (uint32_t)lane * (uint32_t)cNWG;
                int s_ = -1;
                if (c < nCh) {                                  // largest s with cumW[s] <= first step of the chunk
                    const uint32_t t0 = c * CS;
                    int lo_ = 0, hi_ = nsl;
                    while (hi_ - lo_ > 1) { const int mid_ = (lo_ + hi_) >> 1; if (CUMW(mid_) <= t0) lo_ = mid_; else hi_ = mid_; }
                    s_ = lo_;
                }
                sh.sS[w][lane] = s_;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < WIDE_KW; ++k) {                 // pieces (chunk c, slice s_) have id c + s_
                const int s_ = gw + k * NWG;
                pcf[k] = 0u; pcn[k] = 0u;
                if (k < kw && s_ < nsl) {
                    const uint32_t a0 = CUMW(s_), e0 = CUMW(s_ + 1);
                    if (e0 > a0) { pcf[k] = a0 / CS + (uint32_t)s_; pcn[k] = (e0 - 1u) / CS - a0 / CS + 1u; }
                }
            }
        };
        auto full_stream = [&]() {                              // cw <- the layout's own slice bases
            __syncthreads();
            for (int p = ltid; p <= nsl; p += WIDE_NT) cw[p] = p < nsl ? MEMW(p) : Tfull;
            T = Tfull; cmode = 0; cNWG = NWG; cgw = gw;
            geometry();
        };
        auto copy_stream = [&]() {                              // cw <- prefix of the copy's slice widths (wNew, written by its compaction)
            __syncthreads();
            if (w == 0) {
                uint32_t run = 0u;
                for (int p0 = 0; p0 < nsl; p0 += WAVE) {
                    const uint32_t wv = (p0 + lane < nsl) ? __hip_atomic_load(wNew + p0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                    const uint32_t inc = wave_incl_scan(wv);
                    if (p0 + lane < nsl) cw[p0 + lane] = run + inc - wv;
                    run += (uint32_t)__shfl((int)inc, 63);
                }
                if (lane == 0) cw[nsl] = run;
            }
            __syncthreads();
            T = cw[nsl]; Tcopy = T; cmode = 1; cNWG = NWG; cgw = gw;
            geometry();
        };
        full_stream();

        int status = ROMAN_ST_OK;
        roman_stats_t S;
        S.n_assoc_in = pd.nA; S.n_live = L; S.nnz_upper = (int64_t)st[b].nnzUpper;
        S.n_pass = 0; S.outer_iters = 0; S.inner_iters = 0; S.ls_trials = 0; S.score = 0.0; S.d_final = 0.0;
        if (pd.n1 == 0 || pd.n2 == 0) status |= ROMAN_ST_EMPTY_MAP;
        double F = 0.0, d = 0.0, usum = 0.0;
        int n_pass = 0, ls_trials = 0, inner_iters = 0, i = 0;

        // owned elements (registers) and the pieces of their slices
        double u[WIDE_KW], Mu[WIDE_KW], Cu[WIDE_KW], sd[WIDE_KW], tt[WIDE_KW], Mn[WIDE_KW], Cn[WIDE_KW], tb[WIDE_KW], ta[WIDE_KW];
        int kk[WIDE_KW]; bool in[WIDE_KW];
#pragma unroll
        for (int k = 0; k < WIDE_KW; ++k) {
            const int s_ = gw + k * NWG;
            const int pos = (s_ << 6) + lane;
            in[k] = k < kw && pos < L;
            kk[k] = in[k] ? (int)perm[pos] : 0;
            sd[k] = in[k] ? ld[lo + kk[k]] : 0.0;
            const int a_ = in[k] ? lp[lo + kk[k]] : 0;
            if (in[k]) plp[lo + pos] = a_;
            u[k] = in[k] ? (u0 ? u0[lo + a_] : 1.0) : 0.0;
            Mu[k] = Cu[k] = tt[k] = Mn[k] = Cn[k] = tb[k] = ta[k] = 0.0;
        }
        double dummy1[1] = {0.0};
        bool alive = true;
#ifdef ROMAN_SOLVE_TIMING
        unsigned long long wacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wcnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        unsigned long long wlast = wall_clock64();
#define WMARK(slot) do { const unsigned long long t__ = wall_clock64(); wacc[slot] += t__ - wlast; wcnt[slot] += 1; wlast = t__; } while (0)
#else
#define WMARK(slot) do { } while (0)
#endif

        // x (one value per owned element) -> the vector other compute units gather from (by position, like the column labels)
        // together with its support bit map: one ballot word per wave and round (a wave owns 64 consecutive positions)
        auto publish = [&](double* xv, unsigned long long* bm, const double (&x)[WIDE_KW]) {
            FORK(k) {
                if (in[k]) st_pub(xv + (((gw + k * NWG) << 6) + lane), x[k]);
                const unsigned long long m_ = __ballot(in[k] && x[k] > 0.0);
                if (lane == 0 && gw + k * NWG < nsl) __hip_atomic_store(bm + (gw + k * NWG), m_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        // one piece [t, stop) of slice s: partial row sums -> partials buffer.  Blocks of WIDE_U quads (three 16-byte loads
        // per lane and quad), the next block's matrix loads in flight while the current block gathers and accumulates.
        constexpr bool W16 = sizeof(IdxT) == 2;                  // 16-bit column words: 8 bytes per lane and quad, no C flag, 0xffff = no column
        // (the half copy's code costs the whole kernel 20 registers and 220 bytes of scratch per lane — several us per pass of EVERY problem
        //   —: an instantiation of its own, taken where the copy saves more than that: teams on live sets of >= 8 000)
        constexpr bool HALF_ON = HALF && W16;
        typedef typename std::conditional<W16, unsigned long long, uint4_t>::type cword_t;
        auto piece = [&](const double* xv, uint32_t nl, uint32_t tm /* first step in memory */, uint32_t n /* steps */, uint32_t pid) {
            double am = 0.0, ac = 0.0;
            const cword_t* cp = reinterpret_cast<const cword_t*>(cmode ? (const IdxT*)colsK : cols) + (size_t)tm * 64 + lane;
            const dbl2_t* vp = reinterpret_cast<const dbl2_t*>(cmode ? (const double*)valsK : vals) + (size_t)tm * 128 + lane;
            cword_t cA[WIDE_U], cB[WIDE_U]; dbl2_t vA0[WIDE_U], vA1[WIDE_U], vB0[WIDE_U], vB1[WIDE_U];
#define WIDE_ISSUE(C_, V0_, V1_, off_, n_)                                                                    \
            _Pragma("unroll") for (int e = 0; e < WIDE_U; ++e) {                                              \
                const uint32_t q_ = (off_) + min((uint32_t)e, (n_) - 1u);     /* clamped: a repeated quad is skipped by the consumer */ \
                C_[e] = cp[(size_t)q_ * 64]; V0_[e] = vp[(size_t)(2u * q_) * 64]; V1_[e] = vp[(size_t)(2u * q_ + 1u) * 64]; \
            }
#define WIDE_CONSUME(C_, V0_, V1_, n_)                                                                        \
            _Pragma("unroll") for (int e = 0; e < WIDE_U; ++e) {                                              \
                if ((uint32_t)e < (n_)) {                                                                     \
                    uint32_t c4[4];                                                                           \
                    if constexpr (W16) { const unsigned long long cw_ = *reinterpret_cast<const unsigned long long*>(&C_[e]); \
                        c4[0] = (uint32_t)(cw_ & 0xffffu); c4[1] = (uint32_t)((cw_ >> 16) & 0xffffu); c4[2] = (uint32_t)((cw_ >> 32) & 0xffffu); c4[3] = (uint32_t)(cw_ >> 48); } \
                    else { const uint4_t cw_ = *reinterpret_cast<const uint4_t*>(&C_[e]); c4[0] = cw_.x; c4[1] = cw_.y; c4[2] = cw_.z; c4[3] = cw_.w; } \
                    const double v4[4] = {V0_[e].x, V0_[e].y, V1_[e].x, V1_[e].y};                            \
                    _Pragma("unroll") for (int h = 0; h < 4; ++h) {                                           \
                        const uint32_t ci = W16 ? c4[h] : (c4[h] & 0x7fffffffu);                              \
                        double uq = 0.0;                                                                      \
                        if (ci < nl) uq = xl[ci];                                                             \
                        else if (ci < (uint32_t)L && ((bml[ci >> 6] >> (ci & 63u)) & 1ull)) uq = xv[ci];     \
                        am = fma(v4[h], uq, am);                                                              \
                        ac += (!W16 && (c4[h] & 0x80000000u)) ? 0.0 : uq;                                     \
                    }                                                                                         \
                }                                                                                             \
            }
            WIDE_ISSUE(cA, vA0, vA1, 0u, n)
            for (uint32_t o = 0; o < n; o += 2 * WIDE_U) {
                const uint32_t n1 = (n > o + WIDE_U) ? n - o - WIDE_U : 0u;
                if (n1) { WIDE_ISSUE(cB, vB0, vB1, o + WIDE_U, n1) }
                WIDE_CONSUME(cA, vA0, vA1, n - o)
                if (n1) {
                    const uint32_t n2 = (n > o + 2 * WIDE_U) ? n - o - 2 * WIDE_U : 0u;
                    if (n2) { WIDE_ISSUE(cA, vA0, vA1, o + 2 * WIDE_U, n2) }
                    WIDE_CONSUME(cB, vB0, vB1, n1)
                }
            }
#undef WIDE_CONSUME
            double* pp = part + ((size_t)pid * 64 + lane) * 2;
            st_pub(pp, am); st_pub(pp + 1, ac);
        };
        // One piece of my column block of the HALF copy (round 6): a stored entry (p, q, v) serves both (p, q) and (q, p) — pulled
        // into the row's registers ((M x)_p += v x_q, (C x)_p += x_q: x of the block's columns is in LDS, all of it), and pushed
        // into the block's accumulators ((M x)_q += v x_p, (C x)_q += x_p: two ds_add_u64 of fixed-point terms rint(. 2^s), s from the
        // vector's largest element so that a column's sum stays below 2^62 — integer sums: no order, k_solve_up's "exact accumulation").
        // Column labels of the copy are relative to the block's first column; 0xffff (>= Wc) is padding.
        auto piece_up = [&](const double* xv, int s_, uint32_t tm /* first step in the mirror pools */, uint32_t n /* steps */, uint32_t pid, double fxScale, int Wc, const uint16_t* rowAt /* my block's row order */) {
            if constexpr (HALF_ON) {
            const uint32_t rp = (uint32_t)rowAt[((size_t)s_ << 6) + lane];       // (a slice of the block's own order: the lane's row is looked up)
            const double xr = rp < (uint32_t)L ? xv[rp] : 0.0;
            const cword_t* cp = reinterpret_cast<const cword_t*>((const IdxT*)colsK) + (size_t)tm * 64 + lane;
            const dbl2_t* vp = reinterpret_cast<const dbl2_t*>((const double*)valsK) + (size_t)tm * 128 + lane;
            cword_t cA[WIDE_U], cB[WIDE_U]; dbl2_t vA0[WIDE_U], vA1[WIDE_U], vB0[WIDE_U], vB1[WIDE_U];
            WIDE_ISSUE(cA, vA0, vA1, 0u, n)
            double am = 0.0, ac = 0.0;
            const double xrS = xr * fxScale;
            const unsigned long long fC = (unsigned long long)__double_as_longlong(xrS + FX_MAGIC) - FX_MAGIC_BITS;
            const bool push = xr > 0.0;
            l_vec_cp xloc = (l_vec_cp)xl;
            l_acc_p aM = (l_acc_p)(xl + Wc), aC = (l_acc_p)(xl + 2 * Wc);
#define WIDE_CONSUME_UP(C_, V0_, V1_, n_)                                                                     \
            _Pragma("unroll") for (int e = 0; e < WIDE_U; ++e) {                                              \
                if ((uint32_t)e < (n_)) {                                                                     \
                    const unsigned long long cw_ = *reinterpret_cast<const unsigned long long*>(&C_[e]);      \
                    const uint32_t c4[4] = {(uint32_t)(cw_ & 0xffffu), (uint32_t)((cw_ >> 16) & 0xffffu), (uint32_t)((cw_ >> 32) & 0xffffu), (uint32_t)(cw_ >> 48)}; \
                    const double v4[4] = {V0_[e].x, V0_[e].y, V1_[e].x, V1_[e].y};                            \
                    _Pragma("unroll") for (int h = 0; h < 4; ++h) {                                           \
                        if (c4[h] < (uint32_t)Wc) {                                                           \
                            const double uq = xloc[c4[h]];                                                    \
                            am = fma(v4[h], uq, am); ac += uq;                                                \
                            if (push) {                                                                       \
                                __hip_atomic_fetch_add(aM + c4[h], (unsigned long long)__double_as_longlong(fma(v4[h], xrS, FX_MAGIC)) - FX_MAGIC_BITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
                                __hip_atomic_fetch_add(aC + c4[h], fC, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
                            }                                                                                 \
                        }                                                                                     \
                    }                                                                                         \
                }                                                                                             \
            }
            for (uint32_t o = 0; o < n; o += 2 * WIDE_U) {
                const uint32_t n1 = (n > o + WIDE_U) ? n - o - WIDE_U : 0u;
                if (n1) { WIDE_ISSUE(cB, vB0, vB1, o + WIDE_U, n1) }
                WIDE_CONSUME_UP(cA, vA0, vA1, n - o)
                if (n1) {
                    const uint32_t n2 = (n > o + 2 * WIDE_U) ? n - o - 2 * WIDE_U : 0u;
                    if (n2) { WIDE_ISSUE(cA, vA0, vA1, o + 2 * WIDE_U, n2) }
                    WIDE_CONSUME_UP(cB, vB0, vB1, n1)
                }
            }
#undef WIDE_CONSUME_UP
            double* pp = part + ((size_t)pid * 64 + lane) * 2;
            st_pub(pp, am); st_pub(pp + 1, ac);
            }
        };
#undef WIDE_ISSUE
        // Where the gathered values come from.  A 320 KB vector against a 32 KB L1 makes every gather an L2 access, and the
        // whole device does 280 G of those per second: 150 us for the 42 M entries of the n = m = 200 problem, more than
        // the matrix stream itself.  So every workgroup first copies into LDS (a) the support bit map of x (one bit per
        // position) and (b) the leading min(mp1, xcap) elements of x — positions are ranks by degree, so the leading
        // elements are the columns most entries point at, and the support collapses onto them within a few passes.  A
        // gather is then an LDS read; only a column beyond the LDS part whose bit is set goes to L2.
        // Column compaction (round 4).  The iterate's support collapses in plateaus (n = m = 200, method 'gravity': 40 000 -> 22 000
        // for 67 passes -> 3 800 for 89 -> 655 for 29 -> ~100 for 57) while its LARGEST position stays high, so streaming a prefix
        // of the rows gains nothing; but a pass only needs the entries whose COLUMN is in the support.  Every workgroup sees the
        // published support bit map anyway: it keeps the union of the supports multiplied during a window of `cwin` passes, and
        // when that union has fallen to `cthr`/256 of the columns in use the team rewrites the matrix without the other columns —
        // a wave per slice, every lane packs its row's kept entries to the front of the slice (same slice bases, in a mirror of
        // the matrix pools; a compacted copy is compacted again in place), the new widths go through one barrier — and streams
        // the copy for every vector whose support lies in the copy's columns.  A vector that leaves them (the line search can
        // re-admit an element) is multiplied with the full matrix, the copy stays; a window that stayed inside the copy and has
        // shrunk again compacts the copy in place, one that left it twice or more makes a new copy from the full matrix.
        // Dropped entries multiplied zeros: the products are the same up to the grouping of the partial sums (pieces are cut
        // from the shorter stream).
        auto slice_compact = [&](int s_, const IdxT* srcC, const double* srcV) {
            const uint32_t ms = MEMW(s_), nst = CUMW(s_ + 1) - CUMW(s_);
            const cword_t* cp = reinterpret_cast<const cword_t*>(srcC) + (size_t)ms * 64 + lane;
            const dbl2_t* vp = reinterpret_cast<const dbl2_t*>(srcV) + (size_t)ms * 128 + lane;
            cword_t* cq = reinterpret_cast<cword_t*>(colsK) + (size_t)ms * 64 + lane;
            dbl2_t* vq = reinterpret_cast<dbl2_t*>(valsK) + (size_t)ms * 128 + lane;
            const uint32_t inert = W16 ? 0xffffu : ((uint32_t)((s_ << 6) + lane) | 0x80000000u);     // fb_inert of this lane's row
            uint32_t kc = 0u, pc[4] = {inert, inert, inert, inert}; double pv[4] = {0.0, 0.0, 0.0, 0.0};
            auto put = [&](uint32_t q_) {                        // the pending quad -> quad q_ of this lane
                if constexpr (W16) cq[(size_t)q_ * 64] = (unsigned long long)pc[0] | ((unsigned long long)pc[1] << 16) | ((unsigned long long)pc[2] << 32) | ((unsigned long long)pc[3] << 48);
                else { uint4_t o_; o_.x = pc[0]; o_.y = pc[1]; o_.z = pc[2]; o_.w = pc[3]; cq[(size_t)q_ * 64] = o_; }
                vq[(size_t)(2u * q_) * 64] = dbl2_t{pv[0], pv[1]}; vq[(size_t)(2u * q_ + 1u) * 64] = dbl2_t{pv[2], pv[3]};
            };
            // (a wave walks its slice alone, step by step: WIDE_CD steps of loads in flight — one step ahead, the walk of the widest slices, a
            //  thousand dependent round trips, WAS the compaction: 560 us per copy of the n = m = 200 matrix, 0.76 TB/s)
            constexpr int WIDE_CD = 4;
            cword_t cR[WIDE_CD]; dbl2_t aR[WIDE_CD], bR[WIDE_CD];
#pragma unroll
            for (int d = 0; d < WIDE_CD; ++d) {
                cR[d] = cword_t{}; aR[d] = dbl2_t{0.0, 0.0}; bR[d] = dbl2_t{0.0, 0.0};
                if ((uint32_t)d < nst) { cR[d] = cp[(size_t)d * 64]; aR[d] = vp[(size_t)(2 * d) * 64]; bR[d] = vp[(size_t)(2 * d + 1) * 64]; }
            }
            for (uint32_t g0 = 0; g0 < nst; g0 += WIDE_CD) {
#pragma unroll
                for (int d = 0; d < WIDE_CD; ++d) {
                    const uint32_t g = g0 + (uint32_t)d;
                    if (g < nst) {
                        const cword_t cC = cR[d]; const dbl2_t v0 = aR[d], v1 = bR[d];
                        if (g + WIDE_CD < nst) { cR[d] = cp[(size_t)(g + WIDE_CD) * 64]; aR[d] = vp[(size_t)(2u * (g + WIDE_CD)) * 64]; bR[d] = vp[(size_t)(2u * (g + WIDE_CD) + 1u) * 64]; }
                        uint32_t c4[4];
                        if constexpr (W16) { const unsigned long long cw_ = *reinterpret_cast<const unsigned long long*>(&cC);
                            c4[0] = (uint32_t)(cw_ & 0xffffu); c4[1] = (uint32_t)((cw_ >> 16) & 0xffffu); c4[2] = (uint32_t)((cw_ >> 32) & 0xffffu); c4[3] = (uint32_t)(cw_ >> 48); }
                        else { const uint4_t cw_ = *reinterpret_cast<const uint4_t*>(&cC); c4[0] = cw_.x; c4[1] = cw_.y; c4[2] = cw_.z; c4[3] = cw_.w; }
                        const double v4[4] = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
                        for (int h = 0; h < 4; ++h) {
                            const uint32_t ci = W16 ? c4[h] : (c4[h] & 0x7fffffffu);
                            // (an inert slot: 0xffff, or flagged with value 0 — a real flagged entry has a non-zero value)
                            const bool real = W16 ? (ci != 0xffffu) : !((c4[h] & 0x80000000u) && v4[h] == 0.0);
                            if (real && ci < (uint32_t)L && ((bmA[ci >> 6] >> (ci & 63u)) & 1ull)) {
                                const uint32_t j_ = kc & 3u;
#pragma unroll
                                for (int z = 0; z < 4; ++z) if ((uint32_t)z == j_) { pc[z] = c4[h]; pv[z] = v4[h]; }
                                ++kc;
                                if ((kc & 3u) == 0u) {
                                    put((kc >> 2) - 1u);
#pragma unroll
                                    for (int z = 0; z < 4; ++z) { pc[z] = inert; pv[z] = 0.0; }
                                }
                            }
                        }
                    }
                }
            }
            if (kc & 3u) {
                put(kc >> 2);
#pragma unroll
                for (int z = 0; z < 4; ++z) { pc[z] = inert; pv[z] = 0.0; }
            }
            const uint32_t nq = (kc + 3u) >> 2;
            uint32_t wmax = nq;
            for (int off = 32; off > 0; off >>= 1) wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, off));
            for (uint32_t q_ = nq; q_ < wmax; ++q_) put(q_);     // (pending quad is inert here)
            if (lane == 0) __hip_atomic_store(wNew + s_, wmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        // Where the gathered values come from.  A 320 KB vector against a 32 KB L1 makes every gather an L2 access, and the
        // whole device does 280 G of those per second: 150 us for the 42 M entries of the n = m = 200 problem, more than
        // the matrix stream itself.  So every workgroup first copies into LDS (a) the support bit map of x (one bit per
        // position) and (b) the leading min(mp1, xcap) elements of x — positions are ranks by degree, so the leading
        // elements are the columns most entries point at, and the support collapses onto them within a few passes.  A
        // gather is then an LDS read; only a column beyond the LDS part whose bit is set goes to L2.
        auto stream = [&](const double* xv, const unsigned long long* bm, uint32_t mp1, double xmax /* largest element of xv */) -> bool {
            const uint32_t nl = min(mp1, (uint32_t)xcap);
            for (uint32_t p = (uint32_t)ltid; p < (uint32_t)nsl; p += WIDE_NT) bml[p] = bm[p];
            const bool upIn = upOn;
            if (!upOn) for (uint32_t p = (uint32_t)ltid; p < nl; p += WIDE_NT) xl[p] = xv[p];
            if (cmax > 0 && Tfull >= 16u * (uint32_t)NWG) {     // support bookkeeping: the same words, the same verdict in every workgroup of the team
                // (a matrix of fewer than 16 steps per wave is not worth a copy: its passes are barriers, and the books cost 3 us a pass)
                if (ltid == 0) { sh.sint[0] = 0; sh.sint[1] = 0; sh.sint[2] = 0; }
                __syncthreads();
                const bool wend = winPass + 1 >= cwin;          // this pass closes a window
                {
                    int out_ = 0, outA = 0, c_ = 0;
                    for (uint32_t p = (uint32_t)ltid; p < (uint32_t)nsl; p += WIDE_NT) {
                        const unsigned long long w_ = bml[p], a_ = (winPass == 0 ? 0ull : bmA[p]) | w_, c0 = haveCopy ? bmC[p] : 0ull;
                        bmA[p] = a_;
                        if (w_ & ~c0) out_ = 1;
                        if (a_ & ~c0) outA = 1;
                        if (wend) c_ += __popcll(a_);
                    }
                    if (out_ | outA) atomicOr(&sh.sint[0], out_ | (outA << 1));
                    if (wend) {
                        for (int off = 32; off > 0; off >>= 1) c_ += __shfl_xor(c_, off);
                        if (lane == 0 && c_) atomicAdd(&sh.sint[1], c_);
                    }
                }
                __syncthreads();
                bool fits = haveCopy && !(sh.sint[0] & 1);      // the vector's support lies in the copy's columns
                ++winPass;
                if (haveCopy && !fits) ++winOut;
                int doc = 0;                                     // 1: compact the copy in place, 2: a new copy from the full matrix
                const uint32_t cntA = (uint32_t)sh.sint[1];
                if (wend) {
                    const bool sub = haveCopy && !(sh.sint[0] & 2);          // the whole window stayed inside the copy
                    if (ncomp < cmax) {
                        if (sub) { if ((unsigned long long)cntA * 256ull <= (unsigned long long)copyCols * (unsigned long long)cthr && Tcopy >= 16u * (uint32_t)NWG) doc = 1; }
                        else if ((!haveCopy || winOut >= 2) && (unsigned long long)cntA * 256ull <= (unsigned long long)L * (unsigned long long)cthr) doc = 2;
                    }
                    winPass = 0; winOut = 0;
                }
#ifdef ROMAN_SOLVE_TIMING
                const unsigned long long tc0_ = wall_clock64();
#endif
                if (doc) {
                    if (doc == 1 && cmode == 0) copy_stream();  // (slice_compact reads the source's widths from cw)
                    if (doc == 2 && cmode != 0) full_stream();
                    upOn = false;                               // (the compacted copy takes the mirror pools: the half copy is gone)
                    const IdxT* srcC = doc == 1 ? (const IdxT*)colsK : cols; const double* srcV = doc == 1 ? (const double*)valsK : vals;
                    for (int s_ = gw; s_ < nsl; s_ += NWG) slice_compact(s_, srcC, srcV);
                    for (uint32_t p = (uint32_t)ltid; p < (uint32_t)nsl; p += WIDE_NT) bmC[p] = bmA[p];
                    if (!wide_sync<true>(sh, wb, ltid)) return false;
                    haveCopy = true; copyCols = cntA; ++ncomp; fits = true;
                    copy_stream();
                } else if (fits != (cmode == 1)) {
                    if (fits) copy_stream(); else full_stream();
                }
#ifdef ROMAN_SOLVE_TIMING
                if (!HALF_ON && doc) { const unsigned long long tc1_ = wall_clock64(); wacc[7] += tc1_ - tc0_; wcnt[7] += 1; wlast += tc1_ - tc0_; }   // (plain kernel: slot 7 = the compactions, taken out of the stream's slot)
                if (!HALF_ON && cmode == 0) wcnt[6] += 1;       // (passes on the full matrix)
#endif
            }
            if (upIn && !upOn) for (uint32_t p = (uint32_t)ltid; p < nl; p += WIDE_NT) xl[p] = xv[p];   // (left the half copy in this very pass)
            double fxScale = 1.0;
            int Wc = 0, jb = 0; uint32_t upSB_ = 0u, upPB_ = 0u; const uint16_t* rowAt = nullptr;
            if (HALF_ON && upOn) {                              // x over my block's columns, all of it; the pass's fixed-point scale
                Wc = uni_i(sh.upI[1]); jb = uni_i(sh.upI[2]); upSB_ = uni((uint32_t)sh.upSB[jb]); upPB_ = uni((uint32_t)sh.upPB[jb]);
                rowAt = reinterpret_cast<const uint16_t*>(upMeta + (size_t)wb.team * (size_t)bmWords * 1800 + (size_t)WIDE_MAXBLK * bmWords) + (size_t)(2 * WIDE_MAXBLK + jb) * ((size_t)bmWords * 64);
                const int c0 = jb * Wc;
                for (int p = ltid; p < Wc; p += WIDE_NT) xl[p] = (c0 + p < L) ? xv[c0 + p] : 0.0;
                // a term v x 2^s (0 <= v <= 1) below 2^tb, a column's sum of fewer than L terms below 2^62
                int e_ = 0;
                if (xmax > 0.0 && xmax < 1.0e300) (void)frexp(xmax, &e_);
                const int tb = min(49, 62 - (32 - __clz((unsigned)max(L - 1, 1))));
                fxScale = ldexp(1.0, tb - e_);
                if (ltid == 0) sh.upFx = ldexp(1.0, e_ - tb);
            }
            __syncthreads();
            auto chunks = [&](auto half_) {                     // (two copies of the loop: the allocator sees one kind of piece in each)
                constexpr bool H_ = decltype(half_)::value;
                for (int j = 0; j < WIDE_MAXCH; ++j) {
                    int s = uni_i(sh.sS[w][j]);
                    if (s >= 0) {
                        const uint32_t c = (uint32_t)cgw + (uint32_t)j * (uint32_t)cNWG;
                        uint32_t t = c * CS;
                        const uint32_t tEnd = min(T, t + CS);
                        uint32_t sEnd = CUMW(s + 1);
                        while (t < tEnd) {
                            const uint32_t stop = min(sEnd, tEnd);
                            if constexpr (H_) piece_up(xv, s, upSB_ + t, stop - t, upPB_ + c + (uint32_t)s, fxScale, Wc, rowAt);
                            else piece(xv, nl, MEMW(s) + (t - CUMW(s)), stop - t, c + (uint32_t)s);
                            t = stop;
                            if (t < tEnd) { do { ++s; sEnd = CUMW(s + 1); } while (sEnd <= t); }
                        }
                    }
                }
            };
            if (HALF_ON && upOn) chunks(std::true_type{}); else chunks(std::false_type{});
            if (HALF_ON && upOn) {                              // my block's pushed sums -> yPart (write-through), accumulators clean for the next pass
                __syncthreads();
                unsigned long long* ys = yPart + ((size_t)wb.team * (size_t)ySlots + (size_t)wb.tRank) * 2 * (size_t)ycap;
                unsigned long long* aM = reinterpret_cast<unsigned long long*>(xl + Wc);
                const int nv = min(Wc, L - jb * Wc);
                for (int p = ltid; p < nv; p += WIDE_NT) {
                    __hip_atomic_store(ys + p, aM[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(ys + ycap + p, aM[Wc + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    aM[p] = 0ull; aM[Wc + p] = 0ull;
                }
            }
            ++n_pass;
            return true;
        };
        // (M x, C x) of the owned rows: the pieces of their slice in ascending order
        auto collect = [&](double (&om)[WIDE_KW], double (&oc)[WIDE_KW]) {
            static_assert(WIDE_KW == 2, "the two owned slices of a wave are collected together");
            // the pieces of BOTH owned slices are loaded together (four of each in flight) and added per slice in ascending order:
            // half as many dependent round trips to the L2 as one slice after the other
            double m_[2] = {0.0, 0.0}, c_[2] = {0.0, 0.0};
            auto add_pieces2 = [&](uint32_t f0, uint32_t n0, uint32_t f1, uint32_t n1) {
                const dbl2_t* p0 = reinterpret_cast<const dbl2_t*>(part) + (size_t)f0 * 64 + lane;
                const dbl2_t* p1 = reinterpret_cast<const dbl2_t*>(part) + (size_t)f1 * 64 + lane;
                const uint32_t nm = max(n0, n1);
                for (uint32_t q0 = 0; q0 < nm; q0 += 4) {
                    dbl2_t x0[4], x1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        x0[e] = p0[(size_t)((q0 + (uint32_t)e < n0) ? q0 + (uint32_t)e : 0u) * 64];
                        x1[e] = p1[(size_t)((q0 + (uint32_t)e < n1) ? q0 + (uint32_t)e : 0u) * 64];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (q0 + (uint32_t)e < n0) { m_[0] += x0[e].x; c_[0] += x0[e].y; }
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (q0 + (uint32_t)e < n1) { m_[1] += x1[e].x; c_[1] += x1[e].y; }
                }
            };
            if (HALF_ON && upOn) {                              // pulled pieces of every block's stream, then the pushed sums of the slices' own columns' block
                // (a slice lies in ONE column block: Wc is a multiple of 64; the pushed sums are loaded first and fly while the pieces are added)
                const int nblk = uni_i(sh.upI[0]), Wc = uni_i(sh.upI[1]); const double fxInv = sh.upFx;
                // a row's pulled pieces: per block the pieces of the slice of the block's order that holds the row, at the row's lane slot there
                const uint2* gPin = reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(upMeta + (size_t)wb.team * (size_t)bmWords * 1800 + (size_t)WIDE_MAXBLK * bmWords) + (size_t)3 * WIDE_MAXBLK * ((size_t)bmWords * 64));
                {   // (both owned rows of a lane together: their records, then their pieces, in flight at once)
                    const int pos0 = (gw << 6) + lane, pos1 = ((gw + NWG) << 6) + lane;
                    const bool on0 = kw > 0 && in[0], on1 = kw > 1 && in[1];
                    for (int j_ = 0; j_ < nblk; ++j_) {
                        const size_t jo = (size_t)j_ * ((size_t)bmWords * 64);
                        const uint2 pin0 = on0 ? gPin[jo + pos0] : make_uint2(0u, 0u), pin1 = on1 ? gPin[jo + pos1] : make_uint2(0u, 0u);
                        const uint32_t n0 = pin0.y & 0xffffu, n1 = pin1.y & 0xffffu;
                        uint32_t nmax = max(n0, n1);
                        for (int off = 32; off > 0; off >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, off));
                        const dbl2_t* p0 = reinterpret_cast<const dbl2_t*>(part) + (size_t)pin0.x * 64 + (pin0.y >> 16);
                        const dbl2_t* p1 = reinterpret_cast<const dbl2_t*>(part) + (size_t)pin1.x * 64 + (pin1.y >> 16);
                        for (uint32_t q0 = 0; q0 < nmax; q0 += 4) {
                            dbl2_t x0[4], x1[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                x0[e] = p0[(size_t)((q0 + (uint32_t)e < n0) ? q0 + (uint32_t)e : 0u) * 64];
                                x1[e] = p1[(size_t)((q0 + (uint32_t)e < n1) ? q0 + (uint32_t)e : 0u) * 64];
                            }
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (q0 + (uint32_t)e < n0) { m_[0] += x0[e].x; c_[0] += x0[e].y; }
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (q0 + (uint32_t)e < n1) { m_[1] += x1[e].x; c_[1] += x1[e].y; }
                        }
                    }
                }
                // (a slice lies in ONE column block: Wc is a multiple of 64)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int pos = ((gw + k * NWG) << 6) + lane;
                    int jr = 0;
#pragma unroll
                    for (int z = 1; z < WIDE_MAXBLK; ++z) jr += (z < nblk && pos >= z * Wc) ? 1 : 0;
                    const bool on_ = k < kw && in[k];
                    const unsigned long long* ys = yPart + ((size_t)wb.team * (size_t)ySlots + (size_t)sh.upCU[on_ ? jr : 0]) * 2 * (size_t)ycap + (on_ ? pos - jr * Wc : 0);
                    const int ng = on_ ? sh.upG[jr] : 0;
                    unsigned long long sm = 0ull, sc = 0ull;
                    for (int g0 = 0; g0 < ng; g0 += 4) {
                        unsigned long long a2[4], b2[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const size_t o_ = (size_t)min(g0 + e, ng - 1) * 2 * (size_t)ycap; a2[e] = ys[o_]; b2[e] = ys[o_ + ycap]; }
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (g0 + e < ng) { sm += a2[e]; sc += b2[e]; }
                    }
                    if (ng > 0) { m_[k] += fx_decode(sm, fxInv); c_[k] += fx_decode(sc, fxInv); }
                }
            } else if (kw < 2) {                                // one owned slice (the whole device on a problem of fewer slices than waves): eight in flight
                const dbl2_t* pp = reinterpret_cast<const dbl2_t*>(part) + (size_t)pcf[0] * 64 + lane;
                for (uint32_t q0 = 0; q0 < pcn[0]; q0 += 8) {
                    dbl2_t x_[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) x_[e] = pp[(size_t)min(q0 + (uint32_t)e, pcn[0] - 1u) * 64];
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (q0 + (uint32_t)e < pcn[0]) { m_[0] += x_[e].x; c_[0] += x_[e].y; }
                }
            } else add_pieces2(pcf[0], pcn[0], pcf[1], pcn[1]);
#pragma unroll
            for (int k = 0; k < 2; ++k) { om[k] = (k < kw && in[k]) ? m_[k] : 0.0; oc[k] = (k < kw && in[k]) ? c_[k] : 0.0; }
        };
        // trial vector max(base + alpha grad(base), 0) of the owned elements, with the partials of sum t^2 and sum t
        auto trial = [&](const double (&ub)[WIDE_KW], const double (&mb)[WIDE_KW], const double (&cb)[WIDE_KW], double us, double alpha,
                         double (&out)[WIDE_KW], double& ss, double& s1, double& mp, double& mx /* largest element: the scale of a pull + push pass */) {
            FORK(k) {
                const double up = ub[k];
                const double g = (((sd[k] + d) * up - d * us) + mb[k]) + cb[k] * d;
                double t = up + alpha * g;
                t = (in[k] && t > 0.0) ? t : 0.0;
                out[k] = t; ss += t * t; s1 += t; mx = fmax(mx, t);
                if (t > 0.0) mp = fmax(mp, (double)(((gw + k * NWG) << 6) + lane + 1));
            }
        };
        // mean of (M u)_p / Cbu_p over the active set, and the two sums F = A + d B is made of — one grid reduction
        auto d_ratio = [&](bool absval, double (&r4)[4]) -> bool {
            r4[0] = r4[1] = r4[2] = r4[3] = 0.0;
            FORK(k) if (in[k]) {
                const double up = u[k], Cbu = (usum - Cu[k]) - up, mdu = Mu[k] + sd[k] * up;
                if (Cbu > P.eps && up > P.eps) { const double r_ = mdu / Cbu; r4[0] += absval ? fabs(r_) : r_; r4[1] += 1.0; }
                r4[2] += up * mdu; r4[3] += up * ((up - usum) + Cu[k]);
            }
            return wide_reduce<4>(r4, sh, slots, wb, ltid);
        };

        // The iteration as a state machine around ONE stream call site (rescale pass / initial pass / line-search trial).
        // A trial costs TWO grid barriers: the one behind the stream, and one that carries the objective of the trial just
        // multiplied TOGETHER with the sums of both vectors that can come next — the backtracked trial from the same base
        // (published to xva) and the first trial from the accepted vector (xvb): whichever the objective selects is
        // already out when the barrier opens.  (The host sends problems with maxiniters < 1 or maxlsiters < 1 to k_solve.)
        // The HALF copy (round 6; `upOn`, cmode 2).  While the iterate's support is wide no column-compacted copy pays (the columns of the
        // early plateau hold three quarters of the entries), but every pair is stored twice.  At the start of a problem the team writes,
        // into the mirror pools, ONE of the two stored copies of every pair (up_keeps: a checkerboard rule — every row keeps about half of
        // its entries) — cut into COLUMN BLOCKS of at most ycap columns, a flat quad stream per block (a slice's rows' entries of block
        // 0, padded to the slice's width there, then the next slice; then block 1 ...), labels relative to the block — and deals the
        // team's workgroups to the blocks in proportion to their steps.  A workgroup keeps ALL of x over its block's columns in LDS
        // next to two fixed-point accumulators per column: its waves pull into the rows' partials as before and push into the
        // accumulators (piece_up); after the stream the accumulators go to yPart, and the owner of a row adds its pulled pieces
        // (every block) and the pushed sums of the workgroups of its own column's block.  10 bytes per stored pair and pass instead
        // of 20 — and 1.08 x the entries in padding: the rows of a block's stream are in the block's OWN order (windows of 512 positions
        // sorted by the number of entries the row keeps in that block: the 64 rows of a slice hold nearly equal numbers; by position a
        // (slice, block) cell was as wide as the longest of 64 binomial counts: 1.43 x with two blocks, 1.5 x with seven) —, + 32 bytes per
        // column and workgroup of the block.  The first column compaction takes the mirror pools (and every pass thereafter the old
        // path).  Measured: the stream of a pass is bandwidth-bound at the same rate either way; 64 x L = 10 000 on teams
        // 39.7 -> 36.6 ms of solve, smaller live sets lose (the rest of a pass is slower in this instantiation).
        auto build_upper = [&]() -> bool {
            if constexpr (HALF_ON) {
            int nblk = 1, Wc = 0, jb = 0, GU = 1, rkU = 0; uint32_t upSteps = 0u;
            if (!(ucfg & 1) || L < 1024 || Tfull < 16u * (uint32_t)NWG || G > ySlots || G < 2) return true;
            const int WcMax = min(ycap, (int)((uint32_t)xcap / 3u) & ~63);
            if (WcMax < 64) return true;
            nblk = (L + WcMax - 1) / WcMax;
            if (nblk > WIDE_MAXBLK || nblk > G) { nblk = 1; return true; }
            Wc = (((L + nblk - 1) / nblk) + 63) & ~63;          // (<= WcMax: a multiple of 64 that is at least L / nblk)
            const int nsl1 = nsl + 1;
            // per team: per block the kept entries of every row, the row's rank in the block's own ROW ORDER (windows of 512 positions sorted by
            // that count: the 64 rows of a slice of the block's stream then hold nearly equal numbers of entries — by position a (slice, block)
            // cell was as wide as the longest of 64 binomial counts, 1.43 x the entries with two blocks), the row at a rank, and where a row's
            // pulled pieces are (first piece, pieces | lane slot << 16)
            const size_t Lcap = (size_t)bmWords * 64;
            uint32_t* upw = upMeta + (size_t)wb.team * (size_t)bmWords * 1800;
            uint16_t* gCnt = reinterpret_cast<uint16_t*>(upw + (size_t)WIDE_MAXBLK * bmWords);
            uint16_t* gRank = gCnt + WIDE_MAXBLK * Lcap;
            uint16_t* gRow = gRank + WIDE_MAXBLK * Lcap;
            uint2* gPin = reinterpret_cast<uint2*>(gRow + WIDE_MAXBLK * Lcap);
            // which of the two stored copies of a pair the half copy keeps: (p, q) with p < q when p + q is odd, with p > q when it is even —
            // every row keeps about half of its entries whatever the positions of its neighbours (by position order alone the rows of a
            // slice keep very different shares, and a slice is as wide as its longest row: 0.92 of the full stream instead of 0.5)
            auto up_keeps = [](uint32_t rp_, uint32_t ci_) -> bool { return ((rp_ + ci_) & 1u) ? (rp_ < ci_) : (rp_ > ci_); };
            auto blk_of = [&](uint32_t ci) -> int { int j_ = 0; _Pragma("unroll") for (int z = 1; z < WIDE_MAXBLK; ++z) j_ += (z < nblk && ci >= (uint32_t)(z * Wc)) ? 1 : 0; return j_; };
            // (1) widths: a wave per slice counts, per lane, the entries the copy keeps per block
            for (int s_ = cgw; s_ < nsl; s_ += NWG) {
                const uint32_t ms = MEMW(s_), nst = CUMW(s_ + 1) - CUMW(s_);
                const unsigned long long* cp = reinterpret_cast<const unsigned long long*>(cols) + (size_t)ms * 64 + lane;
                const uint32_t rp = ((uint32_t)s_ << 6) + (uint32_t)lane;
                uint32_t cnt[WIDE_MAXBLK];
#pragma unroll
                for (int z = 0; z < WIDE_MAXBLK; ++z) cnt[z] = 0u;
                unsigned long long cN = nst > 0u ? cp[0] : ~0ull;
                for (uint32_t g = 0; g < nst; ++g) {
                    const unsigned long long cC = cN;
                    if (g + 1u < nst) cN = cp[(size_t)(g + 1u) * 64];
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const uint32_t ci = (uint32_t)(cC >> (16 * h)) & 0xffffu;
                        if (ci < (uint32_t)L && up_keeps(rp, ci)) {
                            const int j_ = blk_of(ci);
#pragma unroll
                            for (int z = 0; z < WIDE_MAXBLK; ++z) cnt[z] += (z == j_) ? 1u : 0u;
                        }
                    }
                }
#pragma unroll
                for (int z = 0; z < WIDE_MAXBLK; ++z) if (z < nblk) gCnt[(size_t)z * Lcap + rp] = (uint16_t)min(cnt[z], 0xffffu);
            }
            if (!wide_sync<true>(sh, wb, ltid)) return false;
            // (1b) the blocks' row orders: a wave ranks a window of 512 positions of one block by (count descending, position ascending)
            {
                const int nwin = (nsl * 64 + 511) / 512;
                uint16_t* sc = reinterpret_cast<uint16_t*>(xl) + (size_t)w * 512;     // (the gathered vector's region: no stream yet)
                for (int t_ = cgw; t_ < nblk * nwin; t_ += NWG) {
                    const int j_ = t_ / nwin, base = (t_ - j_ * nwin) * 512, nrow = min(512, nsl * 64 - base);
                    uint32_t c_[8];
#pragma unroll
                    for (int i_ = 0; i_ < 8; ++i_) {
                        const int idx = lane + 64 * i_;
                        c_[i_] = idx < nrow ? (uint32_t)gCnt[(size_t)j_ * Lcap + base + idx] : 0u;
                        sc[idx] = (uint16_t)c_[i_];
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    uint32_t rk_[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                    for (int m_ = 0; m_ < nrow; ++m_) {
                        const uint32_t cm = sc[m_];
#pragma unroll
                        for (int i_ = 0; i_ < 8; ++i_) rk_[i_] += (cm > c_[i_] || (cm == c_[i_] && m_ < lane + 64 * i_)) ? 1u : 0u;
                    }
#pragma unroll
                    for (int i_ = 0; i_ < 8; ++i_) {
                        const int idx = lane + 64 * i_;
                        if (idx < nrow) { gRank[(size_t)j_ * Lcap + base + idx] = (uint16_t)(base + rk_[i_]); gRow[(size_t)j_ * Lcap + base + rk_[i_]] = (uint16_t)(base + idx); }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
            }
            if (!wide_sync<true>(sh, wb, ltid)) return false;
            // (2) every workgroup: cumulative widths per block (LDS, in the region of the gathered vector: no stream yet), the deal
            uint32_t* lw = reinterpret_cast<uint32_t*>(xl);     // [block][nsl1]
            if (w < nblk) {
                uint32_t run = 0u;
                for (int p0 = 0; p0 < nsl; p0 += WAVE) {
                    // (a slice of the block's order is as wide as its first row: the windows are sorted by count, eight slices each)
                    const uint32_t wv = (p0 + lane < nsl) ? (((uint32_t)gCnt[(size_t)w * Lcap + gRow[(size_t)w * Lcap + (size_t)(p0 + lane) * 64]] + 3u) >> 2) : 0u;
                    const uint32_t inc = wave_incl_scan(wv);
                    if (p0 + lane < nsl) lw[w * nsl1 + p0 + lane] = run + inc - wv;
                    run += (uint32_t)__shfl((int)inc, 63);
                }
                if (lane == 0) lw[w * nsl1 + nsl] = run;
            }
            __syncthreads();
            if (ltid == 0) {
                unsigned long long Ttot = 0ull; int ne = 0;
                for (int j_ = 0; j_ < nblk; ++j_) { const uint32_t t_ = lw[j_ * nsl1 + nsl]; Ttot += t_; ne += t_ ? 1 : 0; }
                bool ok = Ttot > 0ull && Ttot <= (unsigned long long)Tfull && ne <= G;
                // (the pushed sums a pass writes and reads, 32 bytes per column and workgroup, against the 2560 bytes of a step it saves)
                ok = ok && (unsigned long long)G * (unsigned long long)Wc * 32ull * 2ull <= Ttot * 2560ull;
                int rem = G, cu = 0; unsigned long long remT = Ttot; uint32_t pb = 0u, sb = 0u;
                for (int j_ = 0; j_ < WIDE_MAXBLK; ++j_) {
                    const uint32_t t_ = j_ < nblk ? lw[j_ * nsl1 + nsl] : 0u;
                    sh.upT[j_] = t_; sh.upSB[j_] = sb; sb += t_; sh.upCU[j_] = cu; sh.upPB[j_] = pb; sh.upCS[j_] = 1u; sh.upG[j_] = 0;
                    if (!ok || t_ == 0u) continue;
                    --ne;
                    int g_ = (int)(((unsigned long long)rem * t_ + remT / 2ull) / remT);
                    g_ = max(1, min(g_, rem - ne));
                    sh.upG[j_] = g_; cu += g_; rem -= g_; remT -= t_;
                    const uint32_t cs_ = chunk_steps(t_, (uint32_t)g_ * WIDE_NW);
                    sh.upCS[j_] = cs_; pb += (t_ + cs_ - 1u) / cs_ + (uint32_t)nsl;
                }
                if (((int64_t)pb + 4) * 128 > (int64_t)partStride) ok = false;
                sh.sint[0] = ok ? 1 : 0; sh.sint[1] = (int)min(Ttot, 0x7fffffffull);
            }
            __syncthreads();
            const bool ok = sh.sint[0] != 0;
            upSteps = (uint32_t)sh.sint[1];
            __syncthreads();
            if (!ok) { nblk = 1; return true; }                 // (the same verdict in every workgroup of the team: the same words)
#pragma unroll
            for (int z = 0; z < WIDE_MAXBLK; ++z) if (sh.upG[z] > 0 && wb.tRank >= sh.upCU[z] && wb.tRank < sh.upCU[z] + sh.upG[z]) jb = z;
            GU = sh.upG[jb]; rkU = wb.tRank - sh.upCU[jb];
            // (3) the copy: every lane scatters the entries of its row that the copy keeps to the row's slot in every block's own order — slice
            // rank / 64, lane slot rank % 64 —, pads the slot to that slice's width, and notes where the row's pulled pieces will be
            for (int s_ = cgw; s_ < nsl; s_ += NWG) {
                const uint32_t ms = MEMW(s_), nst = CUMW(s_ + 1) - CUMW(s_);
                const unsigned long long* cp = reinterpret_cast<const unsigned long long*>(cols) + (size_t)ms * 64 + lane;
                const dbl2_t* vp = reinterpret_cast<const dbl2_t*>(vals) + (size_t)ms * 128 + lane;
                uint16_t* cq = reinterpret_cast<uint16_t*>(colsK); double* vq = valsK;
                const uint32_t rp = ((uint32_t)s_ << 6) + (uint32_t)lane;
                uint32_t cur[WIDE_MAXBLK], rkb[WIDE_MAXBLK];
#pragma unroll
                for (int z = 0; z < WIDE_MAXBLK; ++z) { cur[z] = 0u; rkb[z] = z < nblk ? (uint32_t)gRank[(size_t)z * Lcap + rp] : 0u; }
                // (a slot's entries start vl / 64 of the way into it, cyclically: the lanes of a wave do not push to the same few accumulators
                //  in the same instruction)
                auto put = [&](int j_, uint32_t e0_, uint32_t label, double v_) {
                    uint32_t rk_ = 0u;
#pragma unroll
                    for (int z = 0; z < WIDE_MAXBLK; ++z) if (z == j_) rk_ = rkb[z];
                    const uint32_t v_s = rk_ >> 6, vl = rk_ & 63u;
                    const uint32_t a0_ = lw[j_ * nsl1 + v_s], we_ = (lw[j_ * nsl1 + v_s + 1] - a0_) << 2;
                    uint32_t e_ = e0_ + (we_ * vl >> 6);
                    e_ -= e_ >= we_ ? we_ : 0u;
                    const size_t step = (size_t)sh.upSB[j_] + a0_ + (e_ >> 2);
                    const uint32_t h = e_ & 3u;
                    cq[(step * 64 + vl) * 4 + h] = (uint16_t)label;
                    vq[(step * 128 + (size_t)(h >> 1) * 64 + vl) * 2 + (h & 1u)] = v_;
                };
                unsigned long long cN = ~0ull; dbl2_t v0N = dbl2_t{0.0, 0.0}, v1N = dbl2_t{0.0, 0.0};
                if (nst > 0u) { cN = cp[0]; v0N = vp[0]; v1N = vp[64]; }
                for (uint32_t g = 0; g < nst; ++g) {
                    const unsigned long long cC = cN; const dbl2_t v0 = v0N, v1 = v1N;
                    if (g + 1u < nst) { cN = cp[(size_t)(g + 1u) * 64]; v0N = vp[(size_t)(2u * g + 2u) * 64]; v1N = vp[(size_t)(2u * g + 3u) * 64]; }
                    const double v4[4] = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const uint32_t ci = (uint32_t)(cC >> (16 * h)) & 0xffffu;
                        if (ci < (uint32_t)L && up_keeps(rp, ci)) {
                            const int j_ = blk_of(ci);
                            uint32_t e_ = 0u;
#pragma unroll
                            for (int z = 0; z < WIDE_MAXBLK; ++z) if (z == j_) { e_ = cur[z]; cur[z] += 1u; }
                            put(j_, e_, ci - (uint32_t)(j_ * Wc), v4[h]);
                        }
                    }
                }
#pragma unroll
                for (int z = 0; z < WIDE_MAXBLK; ++z) if (z < nblk) {
                    const uint32_t v_s = rkb[z] >> 6, a0 = lw[z * nsl1 + v_s], e0 = lw[z * nsl1 + v_s + 1];
                    const uint32_t we = (e0 - a0) << 2;
                    for (uint32_t e_ = cur[z]; e_ < we; ++e_) put(z, e_, 0xffffu, 0.0);
                    uint32_t f_ = 0u, n_ = 0u;                   // the pieces of the slot's slice: chunks that overlap it
                    if (e0 > a0 && sh.upG[z] > 0) { const uint32_t cs_ = sh.upCS[z]; f_ = sh.upPB[z] + a0 / cs_ + v_s; n_ = (e0 - 1u) / cs_ - a0 / cs_ + 1u; }
                    gPin[(size_t)z * Lcap + rp] = make_uint2(f_, n_ | ((rkb[z] & 63u) << 16));
                }
            }
            __syncthreads();                                    // (every wave is done with the full matrix's widths in cw and with lw)
            for (int p = ltid; p <= nsl; p += WIDE_NT) cw[p] = lw[jb * nsl1 + p];
            __syncthreads();
            for (int p = ltid; p < 2 * Wc; p += WIDE_NT) reinterpret_cast<unsigned long long*>(xl + Wc)[p] = 0ull;
            if (!wide_sync<true>(sh, wb, ltid)) return false;   // the copy is complete (plain stores: release)
            if (ltid == 0) { sh.upI[0] = nblk; sh.upI[1] = Wc; sh.upI[2] = jb; sh.upI[3] = (int)upSteps; }
            T = sh.upT[jb]; cmode = 2; cNWG = GU * WIDE_NW; cgw = w * GU + rkU;
            geometry();
            upOn = true;
            }
            return true;
        };
        enum { PH_RESCALE, PH_INIT, PH_TRIAL };
        if (L > 0) {
            double r4[4] = {0.0, 0.0, 0.0, 0.0};
            double alpha = 1.0, nr = 0.0, s1cur = 0.0;
            int j = 0, k2 = 0;
            const double* xcur = xva; const unsigned long long* bmcur = bma;
            uint32_t mpcur = (uint32_t)L;                       // support bound of the vector in xcur
            double mxcur = 0.0;                                 // ... and its largest element
            auto normalise = [&]() -> bool {                    // u /= |u|, usum = sum u
                double r2[3] = {0.0, 0.0, 0.0};
                FORK(k) { r2[0] += u[k] * u[k]; r2[1] += u[k]; r2[2] = fmax(r2[2], u[k]); }
                if constexpr (HALF_ON) { if (!wide_reduce<3, 1>(r2, sh, slots, wb, ltid)) return false; }
                else { double q2[2] = {r2[0], r2[1]}; if (!wide_reduce<2>(q2, sh, slots, wb, ltid)) return false; r2[0] = q2[0]; r2[1] = q2[1]; }
                const double nr_ = sqrt(r2[0]);
                if (nr_ > 0.0) FORK(k) u[k] /= nr_;
                usum = (nr_ > 0.0) ? r2[1] / nr_ : r2[1];
                mxcur = (nr_ > 0.0) ? (r2[2] / nr_) * 1.0000001 : r2[2];    // (a bound: the division rounds)
                return true;
            };
            int phase = P.rescale_u0 ? PH_RESCALE : PH_INIT;
            if constexpr (HALF_ON) alive = build_upper();
            if (alive && phase == PH_INIT) alive = normalise();
            if (alive) {                                        // the first vector out; the barrier carries its largest element
                publish(xva, bma, u);
                if constexpr (HALF_ON) {
                    double m1[2] = {0.0, 0.0};
                    FORK(k) { m1[0] = fmax(m1[0], u[k]); m1[1] = fmax(m1[1], -u[k]); }
                    alive = wide_reduce<2, 2>(m1, sh, slots, wb, ltid);
                    mxcur = m1[0];
                    if (alive && upOn && m1[1] > 0.0) { upOn = false; full_stream(); }   // (a caller's start vector with negative elements: the pushed sums are unsigned)
                } else alive = wide_reduce<0>(dummy1, sh, slots, wb, ltid);
            }
            while (alive) {
                if (!(alive = stream(xcur, bmcur, mpcur, mxcur))) break;
                WMARK(upOn ? 7 : 2);                            // (timing build: the pull + push passes apart)
                if (!(alive = wide_reduce<0>(dummy1, sh, slots, wb, ltid))) break;
                WMARK(3);
                collect(Mn, Cn);
                if (phase == PH_RESCALE) {                      // u = normalize(M u0 + diag u0)
                    FORK(k) u[k] = in[k] ? Mn[k] + sd[k] * u[k] : 0.0;
                    if (!(alive = normalise())) break;
                    publish(xva, bma, u);
                    if (!(alive = wide_reduce<0>(dummy1, sh, slots, wb, ltid))) break;
                    mpcur = (uint32_t)L;
                    phase = PH_INIT;
                    continue;
                }
                bool new_outer = false;
                if (phase == PH_INIT) {
                    FORK(k) { Mu[k] = Mn[k]; Cu[k] = Cn[k]; }
                    if (!(alive = d_ratio(false, r4))) break;
                    d = (r4[1] > 0.0) ? r4[0] / r4[1] : 0.0;
                    i = 0;
                    if (i >= P.maxoliters) break;
                    new_outer = true;
                } else {                                        // PH_TRIAL: products of the trial vector
                    ++ls_trials;
                    const double unsum = (nr > 0.0) ? s1cur / nr : s1cur;
                    double r6[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // objective, |du|^2, sums of the two candidates, their support bounds, their largest elements
                    FORK(k) {
                        if (nr > 0.0) { tt[k] /= nr; Mn[k] /= nr; Cn[k] /= nr; }
                        const double up = tt[k];
                        const double g = (((sd[k] + d) * up - d * unsum) + Mn[k]) + Cn[k] * d;
                        r6[0] += up * g;
                        const double df = up - u[k]; r6[1] += df * df;
                    }
                    const bool can_back = k2 + 1 < P.maxlsiters, can_next = j + 1 < P.maxiniters;
                    if (can_back) { trial(u, Mu, Cu, usum, alpha * P.beta, tb, r6[2], r6[3], r6[6], r6[8]); publish(xva, bma, tb); }
                    if (can_next) { trial(tt, Mn, Cn, unsum, 1.0, ta, r6[4], r6[5], r6[7], r6[9]); publish(xvb, bmb, ta); }
                    WMARK(4);
                    if constexpr (HALF_ON) { if (!(alive = (wide_reduce<10, 4>(r6, sh, slots, wb, ltid)))) break; }
                    else {                                      // (the largest elements are the half copy's: eight values as before)
                        double r8[8] = {r6[0], r6[1], r6[2], r6[3], r6[4], r6[5], r6[6], r6[7]};
                        if (!(alive = (wide_reduce<8, 2>(r8, sh, slots, wb, ltid)))) break;
#pragma unroll
                        for (int z = 0; z < 8; ++z) r6[z] = r8[z];
                    }
                    WMARK(5);
                    const double Fnew = r6[0], deltaF = Fnew - F;
                    if (deltaF < -P.eps && can_back) {          // backtrack: the shorter step from the same base is already out
                        alpha *= P.beta; ++k2;
                        FORK(k) tt[k] = tb[k];
                        nr = sqrt(r6[2]); s1cur = r6[3]; xcur = xva; bmcur = bma; mpcur = (uint32_t)r6[6]; mxcur = r6[8];
                        continue;
                    }
                    // accept: the trial vector and its products become the current ones
                    const double du = sqrt(r6[1]);
                    F = Fnew; usum = unsum;
                    FORK(k) { u[k] = tt[k]; Mu[k] = Mn[k]; Cu[k] = Cn[k]; }
                    ++inner_iters; ++j;
                    if (!(du < P.tol_u || fabs(deltaF) < P.tol_F || !can_next)) {   // the inner loop goes on: its next trial is already out
                        alpha = 1.0; k2 = 0;
                        FORK(k) tt[k] = ta[k];
                        nr = sqrt(r6[4]); s1cur = r6[5]; xcur = xvb; bmcur = bmb; mpcur = (uint32_t)r6[7]; mxcur = r6[9];
                        continue;
                    }
                    if (!(alive = d_ratio(true, r4))) break;    // end of the inner loop: homotopy update of d
                    if (r4[1] > 0.0) d += r4[0] / r4[1]; else break;
                    ++i;
                    if (i >= P.maxoliters) break;
                    new_outer = true;
                }
                if (new_outer) {                                // first trial of an inner loop: nothing to overlap it with
                    F = r4[2] + d * r4[3];                      // u . gradF at the new d
                    alpha = 1.0; j = 0; k2 = 0;
                    double r2[4] = {0.0, 0.0, 0.0, 0.0};
                    trial(u, Mu, Cu, usum, alpha, tt, r2[0], r2[1], r2[2], r2[3]);
                    publish(xva, bma, tt);
                    WMARK(0);
                    if constexpr (HALF_ON) { if (!(alive = (wide_reduce<4, 2>(r2, sh, slots, wb, ltid)))) break; }
                    else {
                        double r3[3] = {r2[0], r2[1], r2[2]};
                        if (!(alive = (wide_reduce<3, 1>(r3, sh, slots, wb, ltid)))) break;
                        r2[0] = r3[0]; r2[1] = r3[1]; r2[2] = r3[2];
                    }
                    WMARK(1);
                    nr = sqrt(r2[0]); s1cur = r2[1]; xcur = xva; bmcur = bma; mpcur = (uint32_t)r2[2]; mxcur = r2[3];
                    phase = PH_TRIAL;
                }
            }
        }
        if (!alive) return;                                      // a bounded wait expired: give up (the pre-written records say so)
        if (i >= P.maxoliters) status |= ROMAN_ST_MAXITER;
        S.n_pass = n_pass; S.ls_trials = ls_trials; S.inner_iters = inner_iters;
        S.outer_iters = i; S.score = F; S.d_final = d;
#ifdef ROMAN_SOLVE_TIMING
        WMARK(6);
        if (wb.tRank == 0 && ltid == 0 && O.dbg) {              // 100 MHz ticks -> the host prints them as "cycles": x 10 ns
            unsigned long long* dg = O.dbg + (size_t)b * 16;
            for (int t = 0; t < 8; ++t) { dg[t] = wacc[t]; dg[8 + t] = wcnt[t]; }
            dg[8 + 5] = Tfull; dg[8 + 6] = HALF_ON ? (unsigned long long)sh.upI[3] : wcnt[6];            // (steps of the full stream / of the half copy, all blocks)
        }
#endif
#undef WMARK
        // final u by position for the shared tail (plain stores + one release); workgroup 0 selects and writes the pose
        FORK(k) if (in[k]) vU[rb + ((gw + k * NWG) << 6) + lane] = u[k];
        if (!wide_sync<true>(sh, wb, ltid)) return;
        if (wb.tRank == 0)
            finish_one(D, b, pd, feats, assoc, plp, lp, rowPosPool, permPool, O, L > 0 ? vU + rb : nullptr, vS0 + rb,
                       reinterpret_cast<int32_t*>(vS1 + rb), reinterpret_cast<int32_t*>(vS2 + rb), L, rb, lo, F, status, S, sh.red, sh.sint);
#undef CUMW
#undef FORK
    }
}

// k_skipped: result records of the problems that found no workspace (kind 2): ROMAN_ST_WORKSPACE, no associations,
// NaN pose.  One thread per problem.  Runs right before the solver kernels and also resets their problem queues.
// With `fbList` (the whole-device solver is part of the launch): the fallback problems are listed for it (count in
// wideBar line 21, zeroed by the host before this kernel) and their records PRE-WRITTEN as "not finished" (ROMAN_ST_INTERNAL,
// no associations, NaN pose): the solver overwrites a record when it finishes the problem, so a launch that gives up (a
// bounded wait expired) leaves a statement, not stale memory, for every problem it did not get to.
__global__ void __launch_bounds__(256) k_skipped(int B, const ProbDesc* __restrict__ probs, const ProbState* __restrict__ st, SolveOut O,
                                                 int* __restrict__ queue /* the solvers' problem queues (8 ints): cleared here */,
                                                 int32_t* __restrict__ fbList, unsigned* __restrict__ wideBar)
{
    if (blockIdx.x == 0 && threadIdx.x < 8) queue[threadIdx.x] = 0;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && fbList != nullptr && st[b].kind == 1) {
        fbList[atomicAdd(wideBar + 32 * 21, 1u)] = b;
        for (int t = 0; t < 16; ++t) O.T_out[(int64_t)b * 16 + t] = d_nan();
        O.n_assoc_out[b] = 0; O.status_out[b] = ROMAN_ST_INTERNAL; O.nSel[b] = 0;
        if (O.stats_out) { roman_stats_t S{}; S.n_assoc_in = probs[b].nA; S.n_live = st[b].L; O.stats_out[b] = S; }
    }
    if (b >= B || st[b].kind != 2) return;
    for (int t = 0; t < 16; ++t) O.T_out[(int64_t)b * 16 + t] = d_nan();
    O.n_assoc_out[b] = 0; O.status_out[b] = ROMAN_ST_WORKSPACE; O.nSel[b] = 0;
    if (O.stats_out) { roman_stats_t S{}; S.n_assoc_in = probs[b].nA; S.n_live = st[b].L; O.stats_out[b] = S; }
}

// ---------------------------------------------------------------------------------------------
// Multi-solution extraction (roman_mno_batch*, [REF roman/align/object_registration.py:57-86]): the step between two
// solves of the plain-CLIPPER view of a batch.  One workgroup per problem, one pass over the problem's stored entries
// (stream layout: quads of 256 slots, lane = row slot):
//   score    u_s' M_orig u_s / (u_s' u_s) in f64 over the round's nodes — the diagonal the invariant exports (the single
//            score, or 1) plus twice the stored pairs whose two endpoints are nodes, read from the UNMASKED values;
//   record   the round's count, status, pose, statistics and association rows from the solver's per-round block into
//            solution (b, r) of the caller's arrays;
//   mask     the values of those pairs become 0 in the copy the next solve reads; the column words stay as they are
//            (a masked pair remains a consistent pair of weight 0).  maskMode 1 (first round) writes the whole copy,
//            2 zeroes in place, 0 (last round) writes nothing.
// Membership is a bit map over positions in LDS (L <= STREAM_MAXL bits).  Bound by the 2-byte column words of the pass
// (+ 16 bytes per entry in the round that makes the copy).
// ---------------------------------------------------------------------------------------------
struct MnoRound {
    const int32_t* n_assoc; const int32_t* status; const double* T; const roman_stats_t* stats; const int32_t* assoc;   // the solver's block of this round ([B] / [B][kmax][2])
    int32_t* assoc_out; roman_mno_solution_t* sol_out; roman_stats_t* stats_out;                                       // the caller's arrays ([B][K]...)
    int32_t K, r, kmax, maskMode, diagOne;
};
constexpr int MNO_NT = 512;

__global__ void __launch_bounds__(MNO_NT) k_mno_round(int B, MnoRound R, const ProbDesc* __restrict__ probs, const ProbState* __restrict__ st,
                                                      const int32_t* __restrict__ lpAsc, const double* __restrict__ ls, const uint32_t* __restrict__ rowPos,
                                                      const uint32_t* __restrict__ sliceBase, const uint16_t* __restrict__ cols,
                                                      const double* __restrict__ valsOrig, double* __restrict__ valsMasked,
                                                      const int32_t* __restrict__ nodesOrig, const int32_t* __restrict__ nSel, const double* __restrict__ uOut)
{
    __shared__ double uL[STREAM_MAXL];                          // final u by position
    __shared__ unsigned long long bm[STREAM_MAXL / 64];         // the round's nodes, by position
    __shared__ uint32_t sq[STREAM_MAXL / 64 + 1];               // first quad of every slice (+ the total)
    __shared__ double red[2 * (MNO_NT / 64)];
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NWV = MNO_NT / 64;
    const ProbDesc pd = probs[b];
    const ProbState ps = st[b];
    const int64_t lo = pd.liveOff;
    const bool solved = ps.kind == 0 && ps.L > 0 && ps.L <= STREAM_MAXL;
    const int L = solved ? ps.L : 0;
    const int nsel = solved ? min(max(nSel[b], 0), L) : 0;
    const int nsl = (L + 63) >> 6;
    for (int p = tid; p < L; p += MNO_NT) uL[p] = uOut[ps.rowBase + p];
    if (tid < STREAM_MAXL / 64) bm[tid] = 0ull;
    if (tid <= nsl && solved) sq[tid] = tid < nsl ? (sliceBase[lo + tid] >> 8) : (ps.nnzCap >> 8);
    __syncthreads();
    // nodes -> positions: association index -> live index (the live list is ascending) -> position; diagonal part of the quotient
    double num = 0.0, den = 0.0;
    for (int t = tid; t < nsel; t += MNO_NT) {
        const int a = nodesOrig[ps.rowBase + t];
        int lo_ = 0, hi_ = L - 1;
        while (lo_ < hi_) { const int mid = (lo_ + hi_) >> 1; if (lpAsc[lo + mid] < a) lo_ = mid + 1; else hi_ = mid; }
        const int k = lo_;
        const uint32_t p = rowPos[lo + k];
        if (lpAsc[lo + k] == a && p < (uint32_t)L) {
            atomicOr(&bm[p >> 6], 1ull << (p & 63u));
            const double up = uL[p];
            num += (R.diagOne ? 1.0 : ls[lo + k]) * up * up;
            den += up * up;
        }
    }
    __syncthreads();
    // the stored pairs: quad q of the problem's segment holds entries 4g..4g+3 of the 64 rows of its slice
    if (solved && (nsel > 0 || R.maskMode == 1)) {
        const uint32_t Q = sq[nsl];
        const uint16_t* cp = cols + ps.nnzOff;
        const double* vo = valsOrig + ps.nnzOff;
        double* vm = valsMasked ? valsMasked + ps.nnzOff : nullptr;
        int s = 0;
        double off2 = 0.0;
        for (uint32_t q = (uint32_t)w; q < Q; q += NWV) {
            while (s + 1 < nsl && q >= sq[s + 1]) ++s;          // wave-uniform
            const int p = s * 64 + lane;
            const bool rowIn = p < L && ((bm[p >> 6] >> (p & 63)) & 1ull);
            const uint2 cw = *reinterpret_cast<const uint2*>(cp + (size_t)q * 256 + lane * 4);
            unsigned hit = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t lab = ((j < 2 ? cw.x : cw.y) >> (16 * (j & 1))) & 0xffffu, c = lab & 0x7fffu;
                if (rowIn && c < (uint32_t)L && ((bm[c >> 6] >> (c & 63u)) & 1ull)) hit |= 1u << j;
            }
            const size_t v0 = (size_t)q * 256 + lane * 2, v1 = v0 + 128;     // entries 0,1 and 2,3 of this lane
            if (R.maskMode == 1) {
                double2 a0 = *reinterpret_cast<const double2*>(vo + v0), a1 = *reinterpret_cast<const double2*>(vo + v1);
                if (hit) {
                    const double up = uL[p];
                    if (hit & 1u) { off2 += a0.x * up * uL[cw.x & 0x7fffu]; a0.x = 0.0; }
                    if (hit & 2u) { off2 += a0.y * up * uL[(cw.x >> 16) & 0x7fffu]; a0.y = 0.0; }
                    if (hit & 4u) { off2 += a1.x * up * uL[cw.y & 0x7fffu]; a1.x = 0.0; }
                    if (hit & 8u) { off2 += a1.y * up * uL[(cw.y >> 16) & 0x7fffu]; a1.y = 0.0; }
                }
                *reinterpret_cast<double2*>(vm + v0) = a0; *reinterpret_cast<double2*>(vm + v1) = a1;
            } else if (hit) {
                const double up = uL[p];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!(hit & (1u << j))) continue;
                    const uint32_t c = ((j < 2 ? cw.x : cw.y) >> (16 * (j & 1))) & 0x7fffu;
                    const size_t at = (j < 2 ? v0 : v1) + (size_t)(j & 1);
                    off2 += vo[at] * up * uL[c];
                    if (R.maskMode == 2) vm[at] = 0.0;
                }
            }
        }
        num += 2.0 * off2;
    }
    for (int off = 32; off > 0; off >>= 1) { num += __shfl_xor(num, off); den += __shfl_xor(den, off); }
    if (lane == 0) { red[2 * w] = num; red[2 * w + 1] = den; }
    __syncthreads();
    // record
    const int64_t o = (int64_t)b * R.K + R.r;
    const int n = min(max(R.n_assoc[b], 0), R.kmax);
    for (int t = tid; t < 2 * n; t += MNO_NT) R.assoc_out[o * R.kmax * 2 + t] = R.assoc[(int64_t)b * R.kmax * 2 + t];
    if (tid < 16) R.sol_out[o].T[tid] = R.T[(int64_t)b * 16 + tid];
    if (tid == 0) {
        double sn = 0.0, sd = 0.0;
        for (int i = 0; i < NWV; ++i) { sn += red[2 * i]; sd += red[2 * i + 1]; }
        R.sol_out[o].n_assoc = n; R.sol_out[o].status = R.status[b];
        R.sol_out[o].score = (nsel > 0 && sd > 0.0) ? sn / sd : 0.0;
        if (R.stats_out) R.stats_out[o] = R.stats[b];
    }
}

// ---------------------------------------------------------------------------------------------
// standalone pose kernel: T_align on given correspondences (one wave per problem)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_pose(int dim, const double* __restrict__ pts1,
                                             const double* __restrict__ pts2,
                                             const int64_t* __restrict__ corrOff,
                                             double* __restrict__ T_out, int32_t* __restrict__ status_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t o = corrOff[b]; const int k = (int)(corrOff[b + 1] - o);
    if (k < dim) {
        if (lane == 0) { for (int t = 0; t < 16; ++t) T_out[(int64_t)b * 16 + t] = d_nan(); status_out[b] = ROMAN_ST_INSUFFICIENT; }
        return;
    }
    double T[16];
    wave_pose(T, dim, k, lane, [&](int t, double (&a)[3], double (&q)[3]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] = c < dim ? pts1[(o + t) * dim + c] : 0.0; q[c] = c < dim ? pts2[(o + t) * dim + c] : 0.0; }
    });
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < 16; ++t) T_out[(int64_t)b * 16 + t] = T[t];
        status_out[b] = ROMAN_ST_OK;
    }
}

// ---------------------------------------------------------------------------------------------
// k_ransac: RANSAC registration on object centres ([REF roman/align/ransac_reg.py:16-53]; the deterministic procedure of
// DESIGN.md §4.7), one 256-thread workgroup per problem, every round inside the kernel.
//   - both point sets are staged in LDS once (24 bytes per object);
//   - generation: every lane draws and prunes one hypothesis of the round (integer mixing, six LDS point reads); the survivors of
//     a wave are compacted with a ballot into that wave's LDS queue (k_lists' idea);
//   - scoring: as soon as a queue holds 64 survivors the wave scores them, one per lane — the Kabsch fit in registers, then a
//     uniform loop over i (transform P[i] once) and j (compare with Q[j]): every lane reads the same LDS address in a step, a
//     broadcast; count and sum stay in registers.  A round's last, partial set is scored with the idle lanes masked;
//   - argmax: each lane keeps the best key (count, sse, h) it has seen; after a round the keys are reduced over the wave
//     (cross-lane moves) and over the four waves (LDS), and EVERY thread evaluates the stop rule on the same numbers;
//   - output: each wave sweeps a contiguous quarter of the n1*n2 correspondences twice — counts and centroid sums first, then
//     the rows (ballot + running prefix: row-major order) and the centred cross-covariance — and thread 0 forms the pose with
//     write_pose.  The sums cover ALL inliers whatever kmax is; nothing here depends on what else is in the batch.
//   - the pool may be a submap pool: rows of F >= 3 doubles whose columns 0-2 are the centre — only the two
//     staging loops know —, and thread 0 repeats T, n_assoc and status into the split arrays the loop-closure tail reads.
// ---------------------------------------------------------------------------------------------
struct RansacDesc { int64_t off1, off2; int32_t n1, n2; };

constexpr int RANSAC_NT = 256, RANSAC_NW = RANSAC_NT / 64, RANSAC_QCAP = 128;

// output c + 1 of splitmix64 seeded with `seed`
__device__ __forceinline__ uint64_t ransac_draw(uint64_t seed, uint64_t c)
{
    uint64_t z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}

// the three correspondences of hypothesis h
__device__ __forceinline__ void ransac_sample(uint64_t seed, uint64_t nm, uint32_t m, int64_t h, int (&si)[3], int (&sj)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t a = (uint32_t)__umul64hi(ransac_draw(seed, 3ull * (uint64_t)h + (uint64_t)k), nm);   // < nm <= 2^20
        si[k] = (int)(a / m); sj[k] = (int)(a % m);
    }
}

// the prune: distinct indices on both sides, then open3d's edge-length check on the three index pairs
__device__ __forceinline__ bool ransac_keep(const double* sP, const double* sQ, const int (&si)[3], const int (&sj)[3], double edge_len)
{
    if (si[0] == si[1] || si[0] == si[2] || si[1] == si[2] || sj[0] == sj[1] || sj[0] == sj[2] || sj[1] == sj[2]) return false;
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int l = (k + 1) % 3;
        double s2 = 0.0, t2 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a = sP[si[k] * 3 + c] - sP[si[l] * 3 + c], q = sQ[sj[k] * 3 + c] - sQ[sj[l] * 3 + c];
            s2 += a * a; t2 += q * q;
        }
        const double ds = sqrt(s2), dt = sqrt(t2);
        if (ds < dt * edge_len || dt < ds * edge_len) keep = false;
    }
    return keep;
}

// Kabsch fit source -> target of the three sampled pairs: T (row-major 4x4) with T P[i_k] ~ Q[j_k]
__device__ __forceinline__ void ransac_fit(const double* sP, const double* sQ, const int (&si)[3], const int (&sj)[3], double (&T)[16])
{
    double mq[3], mp[3], H[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mq[c] = (sQ[sj[0] * 3 + c] + sQ[sj[1] * 3 + c] + sQ[sj[2] * 3 + c]) / 3.0;
        mp[c] = (sP[si[0] * 3 + c] + sP[si[1] * 3 + c] + sP[si[2] * 3 + c]) / 3.0;
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) H[e] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) H[r * 3 + c] += (sQ[sj[k] * 3 + r] - mq[r]) * (sP[si[k] * 3 + c] - mp[c]);
    write_pose(T, 3, H, mq, mp);
}

// R p + t, and the squared distance to q: ONE expression for the scoring loop and the output sweeps (same bits, same decisions)
__device__ __forceinline__ void ransac_apply(const double (&T)[16], const double* p, double (&tp)[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) tp[r] = T[r * 4] * p[0] + T[r * 4 + 1] * p[1] + T[r * 4 + 2] * p[2] + T[r * 4 + 3];
}
__device__ __forceinline__ double ransac_d2(const double (&tp)[3], const double* q)
{
    const double dx = tp[0] - q[0], dy = tp[1] - q[1], dz = tp[2] - q[2];
    return dx * dx + dy * dy + dz * dz;
}

// higher count, then lower sse, then lower h
__device__ __forceinline__ bool ransac_better(int ca, double sa, int64_t ha, int cb, double sb, int64_t hb)
{
    return ca > cb || (ca == cb && (sa < sb || (sa == sb && ha < hb)));
}

// The split copies of a record's T, n_assoc and status (the arrays k_lc_tail reads: LcIn), each optional.
struct RansacSplit { double* T; int32_t* n_assoc; int32_t* status; };

// one record, every byte of it (the padding behind best_count included: records of equal results are equal as bytes), and the
// split outputs of problem b wherever a record is written: the same T, n_assoc and status
__device__ __forceinline__ void ransac_record(roman_ransac_record_t* rec, const RansacSplit& out, int b, int n_assoc, int status, int64_t n_hyp,
                                              int64_t n_scored, int64_t best_hyp, int best_count, double best_sse, const double* T /* NULL: NaN */)
{
    static_assert(offsetof(roman_ransac_record_t, best_sse) == offsetof(roman_ransac_record_t, best_count) + 8, "one padding word behind best_count");
    rec->n_assoc = n_assoc; rec->status = status; rec->n_hyp = n_hyp; rec->n_scored = n_scored; rec->best_hyp = best_hyp;
    rec->best_count = best_count; (&rec->best_count)[1] = 0; rec->best_sse = best_sse;
    for (int t = 0; t < 16; ++t) rec->T[t] = T ? T[t] : d_nan();
    if (out.T) for (int t = 0; t < 16; ++t) out.T[(int64_t)b * 16 + t] = T ? T[t] : d_nan();
    if (out.n_assoc) out.n_assoc[b] = n_assoc;
    if (out.status) out.status[b] = status;
}

#define RANSAC_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

__global__ void __launch_bounds__(RANSAC_NT) k_ransac(roman_ransac_params_t P, int B, const RansacDesc* __restrict__ probs, const double* __restrict__ pts,
                                                       int F, int kmax, int32_t* __restrict__ assoc_out, roman_ransac_record_t* __restrict__ rec_out,
                                                       int32_t* __restrict__ counts_out, RansacSplit split)
{
    extern __shared__ __attribute__((aligned(16))) double ransac_pts[];   // P (n1 x 3) | Q (n2 x 3)
    __shared__ uint32_t queue[RANSAC_NW][RANSAC_QCAP];          // per wave: survivors of the round, as h - (start of the round)
    __shared__ int wCnt[2][RANSAC_NW];                          // per wave best key of a round (two areas: a round's writes never meet the previous round's reads)
    __shared__ double wSse[2][RANSAC_NW];
    __shared__ long long wHyp[2][RANSAC_NW];
    __shared__ long long wScored[RANSAC_NW];
    __shared__ double sweep[RANSAC_NW][16];                     // output sweeps: per wave (count, sums of either side) / cross-covariance

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (b >= B) return;
    const RansacDesc pd = probs[b];
    const int n = pd.n1, m = pd.n2;
    roman_ransac_record_t* rec = rec_out + b;
    if (n <= 0 || m <= 0) {
        if (tid == 0) ransac_record(rec, split, b, 0, ROMAN_ST_EMPTY_MAP, 0, 0, -1, 0, 0.0, nullptr);
        return;
    }
    double* sP = ransac_pts; double* sQ = ransac_pts + (size_t)n * 3;
    // the centres are columns 0-2 of rows of F doubles (F = 3: a packed pool); no other column is read
    for (int t = tid; t < n * 3; t += RANSAC_NT) sP[t] = pts[(pd.off1 + t / 3) * F + t % 3];
    for (int t = tid; t < m * 3; t += RANSAC_NT) sQ[t] = pts[(pd.off2 + t / 3) * F + t % 3];
    __syncthreads();

    const uint64_t nm = (uint64_t)n * (uint64_t)m;
    const int64_t maxIter = P.max_iteration;
    const double md2 = P.max_dist * P.max_dist;
    int32_t* counts = counts_out ? counts_out + (int64_t)b * maxIter : nullptr;
    const unsigned long long ltmask = (1ull << lane) - 1ull;

    int bc = -1; double bs = 0.0; int64_t bh = -1;             // this lane's best key so far
    int64_t nScoredWave = 0;                                    // wave-uniform
    int64_t done = 0;
    for (int par = 0; ; par ^= 1) {
        const int64_t r0 = done, r1 = (maxIter - r0 < (int64_t)P.round) ? maxIter : r0 + (int64_t)P.round;
        int qn = 0;                                             // wave-uniform: survivors waiting in this wave's queue
        // one queued survivor per lane: fit, score against all n * m correspondences, fold into the lane's best
        auto score = [&](uint32_t hrel, bool valid) {
            const int64_t h = r0 + (int64_t)hrel;
            double T[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) T[t] = 0.0;
            if (valid) {
                int si[3], sj[3];
                ransac_sample(P.seed, nm, (uint32_t)m, h, si, sj);
                ransac_fit(sP, sQ, si, sj, T);
            }
            int cnt = 0; double sse = 0.0;
            for (int i = 0; i < n; ++i) {
                double tp[3];
                ransac_apply(T, sP + i * 3, tp);
#pragma unroll 4
                for (int j = 0; j < m; ++j) {
                    const double d2 = ransac_d2(tp, sQ + j * 3);
                    const bool in = d2 < md2;
                    cnt += in ? 1 : 0; sse += in ? d2 : 0.0;
                }
            }
            if (valid) {
                if (counts) counts[h] = cnt;
                if (ransac_better(cnt, sse, h, bc, bs, bh)) { bc = cnt; bs = sse; bh = h; }
            }
        };
        for (int64_t hb = r0 + (int64_t)w * 64; hb < r1; hb += RANSAC_NT) {      // (hb is wave-uniform)
            const int64_t h = hb + lane;
            bool keep = false;
            if (h < r1) {
                int si[3], sj[3];
                ransac_sample(P.seed, nm, (uint32_t)m, h, si, sj);
                keep = ransac_keep(sP, sQ, si, sj, P.edge_len);
                if (!keep && counts) counts[h] = -1;
            }
            const unsigned long long bm = __ballot(keep);
            if (keep) queue[w][qn + __popcll(bm & ltmask)] = (uint32_t)(h - r0);
            qn += __popcll(bm); nScoredWave += __popcll(bm);
            RANSAC_WAVE_SYNC();
            if (qn >= 64) {                                     // (qn < 64 before the push: at most 127 entries)
                const uint32_t hrel = queue[w][qn - 64 + lane];
                qn -= 64;
                RANSAC_WAVE_SYNC();                             // the next push may rewrite these slots
                score(hrel, true);
            }
        }
        if (qn > 0) {
            const uint32_t hrel = lane < qn ? queue[w][lane] : 0u;
            RANSAC_WAVE_SYNC();
            score(hrel, lane < qn);
        }
        done = r1;
        // the round's best key: over the wave, then over the waves; every thread ends with the same (bc, bs, bh)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oc = __shfl_xor(bc, off); const double os = __shfl_xor(bs, off); const long long oh = __shfl_xor((long long)bh, off);
            if (ransac_better(oc, os, (int64_t)oh, bc, bs, bh)) { bc = oc; bs = os; bh = (int64_t)oh; }
        }
        if (lane == 0) { wCnt[par][w] = bc; wSse[par][w] = bs; wHyp[par][w] = (long long)bh; }
        __syncthreads();
#pragma unroll
        for (int x = 0; x < RANSAC_NW; ++x) {
            const int oc = wCnt[par][x]; const double os = wSse[par][x]; const int64_t oh = (int64_t)wHyp[par][x];
            if (ransac_better(oc, os, oh, bc, bs, bh)) { bc = oc; bs = os; bh = oh; }
        }
        // stop rule on whole rounds
        if (done >= maxIter) break;
        double K = (double)maxIter;
        if (bc > 0) {
            const double f = (double)bc / (double)nm;
            if (f >= 1.0) K = 0.0;
            else {
                const double den = log(1.0 - f * f * f);
                if (den != 0.0) K = fmin((double)maxIter, ceil(log(1.0 - P.confidence) / den));
            }
        }
        if ((double)done >= K) break;
    }
    if (lane == 0) wScored[w] = (long long)nScoredWave;

    // ---- the winner's inliers and the pose on them ----
    if (bh < 0) {                                               // nothing survived the prune
        __syncthreads();
        if (tid == 0) ransac_record(rec, split, b, 0, ROMAN_ST_INSUFFICIENT, done, 0, -1, 0, 0.0, nullptr);
        return;
    }
    double T[16];
    {
        int si[3], sj[3];
        ransac_sample(P.seed, nm, (uint32_t)m, bh, si, sj);
        ransac_fit(sP, sQ, si, sj, T);
    }
    const int64_t len = (int64_t)((nm + RANSAC_NT - 1) / RANSAC_NT) * 64;                 // correspondences per wave, a multiple of 64
    const int64_t a0 = (int64_t)w * len, a1 = a0 + len < (int64_t)nm ? a0 + len : (int64_t)nm;
    auto inlier = [&](int64_t a, int& i, int& j) -> bool {
        if (a >= a1) return false;
        i = (int)((uint32_t)a / (uint32_t)m); j = (int)((uint32_t)a % (uint32_t)m);
        double tp[3];
        ransac_apply(T, sP + i * 3, tp);
        return ransac_d2(tp, sQ + j * 3) < md2;
    };
    int wn = 0;                                                 // wave-uniform: inliers of this wave's range
    double s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
    for (int64_t ab = a0; ab < a1; ab += 64) {
        int i = 0, j = 0;
        const bool in = inlier(ab + lane, i, j);
        wn += __popcll(__ballot(in));
        if (in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { s1[c] += sP[i * 3 + c]; s2[c] += sQ[j * 3 + c]; }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { s1[c] = readlane63(wave_sum63(s1[c])); s2[c] = readlane63(wave_sum63(s2[c])); }
    if (lane == 0) {
        sweep[w][0] = (double)wn;
#pragma unroll
        for (int c = 0; c < 3; ++c) { sweep[w][1 + c] = s1[c]; sweep[w][4 + c] = s2[c]; }
    }
    __syncthreads();
    int total = 0, base = 0;
    double m1[3] = {0, 0, 0}, m2[3] = {0, 0, 0};
#pragma unroll
    for (int x = 0; x < RANSAC_NW; ++x) {
        const int cx = (int)sweep[x][0];
        if (x < w) base += cx;
        total += cx;
#pragma unroll
        for (int c = 0; c < 3; ++c) { m1[c] += sweep[x][1 + c]; m2[c] += sweep[x][4 + c]; }
    }
    if (total > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { m1[c] /= (double)total; m2[c] /= (double)total; }
    }
    __syncthreads();                                            // `sweep` is rewritten below
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int run = base;
    int32_t* rows = assoc_out + (int64_t)b * kmax * 2;
    for (int64_t ab = a0; ab < a1; ab += 64) {
        int i = 0, j = 0;
        const bool in = inlier(ab + lane, i, j);
        const unsigned long long bm = __ballot(in);
        if (in) {
            const int pos = run + __popcll(bm & ltmask);
            if (pos < kmax) { rows[2 * (int64_t)pos] = i; rows[2 * (int64_t)pos + 1] = j; }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) H[r * 3 + c] += (sP[i * 3 + r] - m1[r]) * (sQ[j * 3 + c] - m2[c]);
        }
        run += __popcll(bm);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) H[e] = readlane63(wave_sum63(H[e]));
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) sweep[w][e] = H[e];
    }
    __syncthreads();
    if (tid == 0) {
        long long scored = 0;
        for (int x = 0; x < RANSAC_NW; ++x) scored += wScored[x];
        int status = ROMAN_ST_OK;
        double To[16];
        if (total < 3) {
            status |= ROMAN_ST_INSUFFICIENT;
            for (int t = 0; t < 16; ++t) To[t] = d_nan();
        } else {
            double Hs[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) Hs[e] = ((sweep[0][e] + sweep[1][e]) + sweep[2][e]) + sweep[3][e];
            write_pose(To, 3, Hs, m1, m2);
        }
        if (total > kmax) status |= ROMAN_ST_ASSOC_TRUNCATED;
        ransac_record(rec, split, b, total, status, done, scored, bh, bc, bs, To);
    }
}

// ---------------------------------------------------------------------------------------------
// loop-closure tail: what the caller of the pair loop does with a pose before it reaches the pose graph
// (post-filters, error metrics, acceptance, edge, compaction).  A few hundred f64 operations per problem: launch- and
// latency-bound, one thread per problem; the accepted list comes from k_rowbase's one-workgroup scan.
// ---------------------------------------------------------------------------------------------
struct LcIn {
    const double* T; const int32_t* n_assoc; const int32_t* status;      // batch outputs
    const double* T_ref; const int32_t* enable;                          // optional
    const double* FL; const int32_t* iL; const double* FR; const int32_t* iR;   // optional frame pools
};

// C = A B for row-major 4x4 matrices, left to right as NumPy's `@` chain does
__device__ __forceinline__ void lc_mul4(const double* A, const double* Bm, double* Cm)
{
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += A[r * 4 + k] * Bm[k * 4 + c];
            Cm[r * 4 + c] = s;
        }
}

// inverse of an affine 4x4 (bottom row 0 0 0 1) through the cofactors of its 3x3 block: np.linalg.inv's result for ANY
// invertible block, not only a rotation (the estimate is orthogonal only to rounding)
__device__ __forceinline__ void lc_inv_affine(const double* A, double* I)
{
    const double a = A[0], b = A[1], c = A[2], d = A[4], e = A[5], f = A[6], g = A[8], h = A[9], i = A[10];
    const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
    const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double det = a * c00 + b * c10 + c * c20;
    const double r = 1.0 / det;
    I[0] = c00 * r; I[1] = c01 * r; I[2] = c02 * r;
    I[4] = c10 * r; I[5] = c11 * r; I[6] = c12 * r;
    I[8] = c20 * r; I[9] = c21 * r; I[10] = c22 * r;
    const double tx = A[3], ty = A[7], tz = A[11];
    I[3] = -(I[0] * tx + I[1] * ty + I[2] * tz);
    I[7] = -(I[4] * tx + I[5] * ty + I[6] * tz);
    I[11] = -(I[8] * tx + I[9] * ty + I[10] * tz);
    I[12] = 0.0; I[13] = 0.0; I[14] = 0.0; I[15] = 1.0;
}

// lc_pose_record: the record of ONE pose — what k_lc_tail does per problem and k_mno_lc_tail per (problem, hypothesis).
// GATES compare what the host compares — the angles themselves (roll, pitch from atan2 /
// asin) against the thresholds, the association count against lc_association_thresh — so a decision depends on a library
// function's last bit exactly where the host's does.
// Quaternion: the branch rule of scipy's Rotation.from_matrix — the FIRST maximum of (R00, R11, R22, trace) picks the
// component that is computed as a sum (hence non-negative), the other three follow from it, the vector is normalised and
// NOT canonicalised (w may be negative): as_quat()'s component order xyzw and sign.
// st, T: the pose's status and its 16 doubles; n_assoc, enable, iL, iR: the pose's ENTRIES of those arrays (enable, iL, iR NULL with
// their arrays), read only where the host reads them; T_ref: the problem's 16 doubles or NULL; FL, FR: the frame pools or NULL.
__device__ __forceinline__ void lc_pose_record(const roman_lc_params_t& P, int problem, int st, const double* T, const int32_t* n_assoc,
                                               const double* T_ref, const int32_t* enable, const double* FL, const int32_t* iL,
                                               const double* FR, const int32_t* iR, roman_lc_record_t& R)
{
    int flags = 0;
    if (st & ROMAN_ST_WORKSPACE) flags = ROMAN_LC_SKIPPED;
    else if (st & ROMAN_ST_INTERNAL) flags = ROMAN_LC_INTERNAL;
    else if (st & (ROMAN_ST_INSUFFICIENT | ROMAN_ST_EMPTY_MAP)) flags = ROMAN_LC_FAILED_INSUFFICIENT;
    double Th[16];
    if (!flags) {
        if (P.dim == 2) {                                        // planar estimate lifted to SE(3), identity in z
#pragma unroll
            for (int t = 0; t < 16; ++t) Th[t] = (t % 5 == 0) ? 1.0 : 0.0;
            Th[0] = T[0]; Th[1] = T[1]; Th[4] = T[3]; Th[5] = T[4]; Th[3] = T[2]; Th[7] = T[5];
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) Th[t] = T[t];
            // R = Rz(yaw) Ry(pitch) Rx(roll): the angles of as_euler('ZYX') and, reversed, of the fixed-axis 'xyz'
            const double pitch = -asin(fmin(fmax(Th[8], -1.0), 1.0));
            const double roll = atan2(Th[9], Th[10]);
            if (P.tilt_thresh >= 0.0 && !(fabs(roll) < P.tilt_thresh && fabs(pitch) < P.tilt_thresh)) flags = ROMAN_LC_FAILED_TILT;
            else if (P.force_rm_upside_down) {
                const double half_pi = 90.0 * (3.141592653589793 / 180.0);      // np.deg2rad(90.)
                if (fabs(roll) > half_pi || fabs(pitch) > half_pi) flags = ROMAN_LC_FAILED_UPSIDE_DOWN;
            }
            if (!flags && P.force_rm_lc_roll_pitch) {            // yaw only; the translation stays
                const double yaw = atan2(Th[4], Th[0]);
                const double cy = cos(yaw), sy = sin(yaw);
                Th[0] = cy; Th[1] = -sy; Th[2] = 0.0; Th[4] = sy; Th[5] = cy; Th[6] = 0.0; Th[8] = 0.0; Th[9] = 0.0; Th[10] = 1.0;
            }
        }
    }
    R.problem = problem; R.reserved = 0;
    double theta = 180.0, dist = 1e6;                            // the sentinels of the except-branch
    int n = 0;
    if (!flags) {
        n = *n_assoc;
        theta = d_nan(); dist = d_nan();
        if (T_ref) {
            double Ti[16], E[16];
            lc_inv_affine(Th, Ti);
            lc_mul4(Ti, T_ref, E);
            if (P.dim == 2) { theta = atan2(E[4], E[0]); dist = sqrt(E[3] * E[3] + E[7] * E[7]); }
            else {
                // rotation magnitude: 2 atan2(|q_xyz|, |q_w|) == atan2(|skew part| / 2, (trace - 1) / 2) on [0, pi]
                const double sx = E[9] - E[6], sy = E[2] - E[8], sz = E[4] - E[1];
                theta = atan2(0.5 * sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (E[0] + E[5] + E[10] - 1.0));
                dist = sqrt(E[3] * E[3] + E[7] * E[7] + E[11] * E[11]);
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) Th[t] = d_nan();
    }
    const bool countable = !(flags & (ROMAN_LC_SKIPPED | ROMAN_LC_INTERNAL));
    const bool accepted = countable && n >= P.lc_association_thresh && (!enable || *enable != 0);
    double et[3] = {d_nan(), d_nan(), d_nan()}, eq[4] = {d_nan(), d_nan(), d_nan(), d_nan()};
    if (accepted) {
        flags |= ROMAN_LC_ACCEPTED;
        double A[16], E[16];
        const double* Ep = Th;
        if (FL) { lc_mul4(FL + (int64_t)*iL * 16, Th, A); Ep = A; }
        if (FR) { lc_mul4(Ep, FR + (int64_t)*iR * 16, E); Ep = E; }
        et[0] = Ep[3]; et[1] = Ep[7]; et[2] = Ep[11];
        const double m00 = Ep[0], m11 = Ep[5], m22 = Ep[10], tr = m00 + m11 + m22;
        int choice = 0; double best = m00;
        if (m11 > best) { best = m11; choice = 1; }
        if (m22 > best) { best = m22; choice = 2; }
        if (tr > best) { best = tr; choice = 3; }
        double q[4];
        if (choice == 3) { q[0] = Ep[9] - Ep[6]; q[1] = Ep[2] - Ep[8]; q[2] = Ep[4] - Ep[1]; q[3] = 1.0 + tr; }
        else {
            const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
            q[i] = 1.0 - tr + 2.0 * Ep[i * 4 + i];
            q[j] = Ep[j * 4 + i] + Ep[i * 4 + j];
            q[k] = Ep[k * 4 + i] + Ep[i * 4 + k];
            q[3] = Ep[k * 4 + j] - Ep[j * 4 + k];
        }
        const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
        for (int t = 0; t < 4; ++t) eq[t] = q[t] / nq;
    }
    R.n_assoc = n; R.flags = flags; R.theta = theta; R.dist = dist;
#pragma unroll
    for (int t = 0; t < 16; ++t) R.T_hat[t] = Th[t];
#pragma unroll
    for (int t = 0; t < 3; ++t) R.edge_t[t] = et[t];
#pragma unroll
    for (int t = 0; t < 4; ++t) R.edge_q[t] = eq[t];
}

// k_lc_tail: one record per problem, one thread each.
__global__ void __launch_bounds__(256) k_lc_tail(roman_lc_params_t P, int B, LcIn in, roman_lc_record_t* __restrict__ rec)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    roman_lc_record_t R;
    lc_pose_record(P, b, in.status[b], in.T + (int64_t)b * 16, in.n_assoc + b, in.T_ref ? in.T_ref + (int64_t)b * 16 : nullptr,
                   in.enable ? in.enable + b : nullptr, in.FL, in.iL ? in.iL + b : nullptr, in.FR, in.iR ? in.iR + b : nullptr, R);
    rec[b] = R;
}

// lc_compact: the indices b < B with take(b) in ascending order and their count, by one workgroup; a thread takes PER
// consecutive indices and k_rowbase's block scan places them — deterministic, the order of the reference's edge loop.
template <typename Take>
__device__ __forceinline__ void lc_compact(int B, Take take, int32_t* __restrict__ idx, int32_t* __restrict__ count)
{
    __shared__ int shi[17];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int PER = (B + nt - 1) / nt;
    const int b0 = min(B, tid * PER), b1 = min(B, b0 + PER);
    int mine = 0;
    for (int b = b0; b < b1; ++b) mine += take(b) ? 1 : 0;
    int total;
    int pos = block_excl_scan(mine, shi, total);
    for (int b = b0; b < b1; ++b) if (take(b)) idx[pos++] = b;
    if (tid == 0) *count = total;
}

// k_lc_compact: the accepted records.
__global__ void __launch_bounds__(1024) k_lc_compact(int B, const roman_lc_record_t* __restrict__ rec, int32_t* __restrict__ idx, int32_t* __restrict__ count)
{
    lc_compact(B, [&](int b) { return (rec[b].flags & ROMAN_LC_ACCEPTED) != 0; }, idx, count);
}

// ---------------------------------------------------------------------------------------------
// the tail over K hypotheses per problem (roman_mno_solution_t[B][K]): one wave per problem, lane k builds
// the record of hypothesis k with lc_pose_record — per (b, k) the arithmetic of k_lc_tail — and the wave picks the problem's
// best hypothesis: among the records without a FAILED_*, SKIPPED or INTERNAL flag the largest n_assoc, the lowest k among
// equals; -1 when there is none.  The maximum runs over n_assoc + 1 (0 = no candidate, the neutral element) through the DPP
// tree of wave_max63, the winner is the first set bit of a ballot: no LDS, no atomics, a pure function of the records.
// ---------------------------------------------------------------------------------------------
constexpr int MNO_LC_NT = 256;                                   // four problems per workgroup

__device__ __forceinline__ int wave_max63_i32(int v)            // (of non-negative values; valid in lane 63)
{
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false));     // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false));     // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false));    // row_ror:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false));    // row_ror:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));    // row_bcast:15 -> rows 1,3
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));    // row_bcast:31 -> rows 2,3
    return v;
}

__global__ void __launch_bounds__(MNO_LC_NT) k_mno_lc_tail(roman_lc_params_t P, int B, int K, const roman_mno_solution_t* __restrict__ sol,
                                                            const double* __restrict__ T_ref, const int32_t* __restrict__ enable,
                                                            const double* __restrict__ FL, const int32_t* __restrict__ iL,
                                                            const double* __restrict__ FR, const int32_t* __restrict__ iR,
                                                            roman_lc_record_t* __restrict__ rec, int32_t* __restrict__ best)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (MNO_LC_NT / 64) + (threadIdx.x >> 6);        // wave-uniform
    if (b >= B) return;
    int key = 0;                                                 // n_assoc + 1 of a candidate, 0 otherwise
    if (lane < K) {
        const int64_t r = (int64_t)b * K + lane;
        const roman_mno_solution_t* s = sol + r;
        roman_lc_record_t R;
        lc_pose_record(P, (int)r, s->status, s->T, &s->n_assoc, T_ref ? T_ref + (int64_t)b * 16 : nullptr, enable ? enable + b : nullptr,
                       FL, iL ? iL + b : nullptr, FR, iR ? iR + b : nullptr, R);
        rec[r] = R;
        const int no = ROMAN_LC_FAILED_INSUFFICIENT | ROMAN_LC_FAILED_TILT | ROMAN_LC_FAILED_UPSIDE_DOWN | ROMAN_LC_SKIPPED | ROMAN_LC_INTERNAL;
        if (!(R.flags & no)) key = max(R.n_assoc, 0) + 1;
    }
    const int top = __builtin_amdgcn_readlane(wave_max63_i32(key), 63);
    const unsigned long long won = __ballot(key == top);
    if (lane == 0) best[b] = top > 0 ? __ffsll((long long)won) - 1 : -1;
}

// k_mno_best_compact: the problems whose best hypothesis is accepted, ascending, and their count.
__global__ void __launch_bounds__(1024) k_mno_best_compact(int B, int K, const roman_lc_record_t* __restrict__ rec, const int32_t* __restrict__ best,
                                                           int32_t* __restrict__ idx, int32_t* __restrict__ count)
{
    lc_compact(B, [&](int b) { const int k = best[b]; return k >= 0 && (rec[(int64_t)b * K + k].flags & ROMAN_LC_ACCEPTED) != 0; }, idx, count);
}

// ---------------------------------------------------------------------------------------------
// shared-segment removal for self loop closures: the reference drops from both submaps of a pair every segment whose id
// occurs in both before it registers them ([REF roman/align/submap_align.py:108-115]).  One int64 id per row of the feature
// pool; k_shared_mark lists, per problem and side, the local indices that stay; k_shared_gather copies those rows of the
// problems that lost something into a region behind the pool (the others keep pointing at the pool); k_shared_reduce does both
// in one launch for device-pointer callers, into fixed slots of the region.
// ---------------------------------------------------------------------------------------------
struct ShareDesc { int64_t off1, off2, keep; int32_t n1, n2; };   // keep: start of the problem's slice of the keep lists (side 1, then side 2)
struct GatherJob { int64_t src, dst, keep; int32_t n, pad; };     // one side of an affected problem: pool rows src + keep[.] -> rows dst ..

constexpr int SHARE_TILE = 1024;                                 // ids of the other side staged in LDS at a time (8 KB)

// shared_mark_problem: the mark step of problem b by its workgroup of NT threads (NT = 256, or one wave: NT = 64, every map of
// the call at most 64 objects).  A lane holds one object of its own side and walks the other side's ids, staged in LDS in
// tiles and read as broadcasts (every lane the same address); the comparison is the full 64-bit equality, so every repetition
// of an id inside a map meets the same fate.  Ranks come from the ballot of the survivors plus the counts of the waves in
// front: the list is ascending, no atomics.  -> nKept[side], the same in every thread.
template <int NT>
__device__ __forceinline__ void shared_mark_problem(const ShareDesc& P, int b, const int64_t* __restrict__ ids, int32_t* keep,
                                                    int32_t* __restrict__ kept, int64_t* tile, int* wcnt, int (&nKept)[2])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int side = 0; side < 2; ++side) {
        const int64_t* own = ids + (side ? P.off2 : P.off1); const int nOwn = side ? P.n2 : P.n1;
        const int64_t* oth = ids + (side ? P.off1 : P.off2); const int nOth = side ? P.n1 : P.n2;
        int32_t* out = keep + P.keep + (side ? P.n1 : 0);
        int base = 0;
        for (int i0 = 0; i0 < nOwn; i0 += NT) {                  // (uniform bounds: every barrier below is met by the whole workgroup)
            const int i = i0 + tid;
            const bool valid = i < nOwn;
            const int64_t mine = valid ? own[i] : 0;
            bool found = false;
            for (int t0 = 0; t0 < nOth; t0 += SHARE_TILE) {
                const int tn = min(SHARE_TILE, nOth - t0);
                __syncthreads();                                 // the readers of the previous tile are done
                for (int k = tid; k < tn; k += NT) tile[k] = oth[t0 + k];
                __syncthreads();
#pragma unroll 8
                for (int k = 0; k < tn; ++k) found |= (tile[k] == mine);
            }
            const bool stays = valid && !found;
            const unsigned long long m = __ballot(stays);
            int before = 0, total = __popcll(m);
            if (NT > 64) {
                __syncthreads();                                 // the counts of the previous chunk have been read
                if (lane == 0) wcnt[wave] = total;
                __syncthreads();
                total = 0;
#pragma unroll
                for (int w = 0; w < NT / 64; ++w) { const int cw = wcnt[w]; before += (w < wave) ? cw : 0; total += cw; }
            }
            if (stays) out[base + before + __popcll(m & lt)] = i;
            base += total;
        }
        if (tid == 0) kept[2 * b + side] = base;
        nKept[side] = base;
    }
}

// k_shared_mark: the mark step alone, one workgroup (or one wave) per problem.
template <int NT>
__global__ void __launch_bounds__(NT) k_shared_mark(int B, const ShareDesc* __restrict__ probs, const int64_t* __restrict__ ids,
                                                    int32_t* __restrict__ keep, int32_t* __restrict__ kept)
{
    __shared__ int64_t tile[SHARE_TILE];
    __shared__ int wcnt[NT / 64];
    const int b = blockIdx.x;
    if (b >= B) return;
    const ShareDesc P = probs[b];
    int nKept[2];
    shared_mark_problem<NT>(P, b, ids, keep, kept, tile, wcnt, nKept);
}

// copy_row: F doubles of one row as 64-bit words by one wave, lanes along the row (bit for bit): V2 (F even, 16-byte aligned
// base: every row is then 16-byte aligned) moves 16 bytes per lane, otherwise 8.
template <bool V2>
__device__ __forceinline__ void copy_row(unsigned long long* __restrict__ d, const unsigned long long* __restrict__ s, int F, int lane)
{
    if (V2) {
        const ulonglong2* s2 = reinterpret_cast<const ulonglong2*>(s);
        ulonglong2* d2 = reinterpret_cast<ulonglong2*>(d);
        for (int k = lane; k < (F >> 1); k += 64) d2[k] = s2[k];
    } else {
        for (int k = lane; k < F; k += 64) d[k] = s[k];
    }
}

// k_shared_reduce: mark and gather of one problem in ONE launch, one workgroup (NT = 256) or one wave (NT = 64) per problem: the
// host places nothing by a count.  The mark step is shared_mark_problem; behind a workgroup barrier (the keep entries the
// workgroup wrote are then visible to all its waves) a problem that lost an object on either side copies the kept rows of both
// sides, in list order, into its FIXED slots of the gather region behind the pool: side 1 at rows region_row0 + P.keep ..,
// side 2 at rows region_row0 + P.keep + n1 .. — the slot offset is the keep-list offset.  A problem that lost nothing writes no
// row; rows of a slot behind the kept ones are not written.  Every wave of the workgroup copies (a wave per row): at demo scale a
// row is about 6 KB and the copy, not the mark, is the time.  `feats`: pool rows, then the region (the pool slices lie in front
// of region_row0, so no row is read and written).
template <int NT, bool V2>
__global__ void __launch_bounds__(NT) k_shared_reduce(int B, int F, const ShareDesc* __restrict__ probs, const int64_t* __restrict__ ids,
                                                      int32_t* keep, int32_t* __restrict__ kept, unsigned long long* feats, int64_t region_row0)
{
    __shared__ int64_t tile[SHARE_TILE];
    __shared__ int wcnt[NT / 64];
    const int b = blockIdx.x;
    if (b >= B) return;
    const ShareDesc P = probs[b];
    int nKept[2];
    shared_mark_problem<NT>(P, b, ids, keep, kept, tile, wcnt, nKept);
    if (nKept[0] == P.n1 && nKept[1] == P.n2) return;            // (uniform) nothing lost: the problem reads the pool as given
    __syncthreads();                                             // the keep lists of this workgroup are written and visible
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int side = 0; side < 2; ++side) {
        const int64_t src = side ? P.off2 : P.off1, slot = P.keep + (side ? P.n1 : 0);
        const int32_t* list = keep + slot;
        for (int r = wave; r < nKept[side]; r += NT / 64)
            copy_row<V2>(feats + (region_row0 + slot + r) * (int64_t)F, feats + (src + list[r]) * (int64_t)F, F, lane);
    }
}

// k_shared_gather: the kept rows of one side of an affected problem, in order, F doubles per row moved as 64-bit words (bit for
// bit).  A wave per row, lanes along the row: V2 (F even: every row of the pool and of the gather region is 16-byte aligned)
// moves 16 bytes per lane, otherwise 8.  grid (jobs, row groups).
template <bool V2>
__global__ void __launch_bounds__(256) k_shared_gather(int F, const GatherJob* __restrict__ jobs, const int32_t* __restrict__ keep,
                                                       unsigned long long* pool)
{
    const GatherJob J = jobs[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.y * 4 + wave; r < J.n; r += 4 * gridDim.y) {
        const unsigned long long* s = pool + (J.src + keep[J.keep + r]) * (int64_t)F;
        unsigned long long* d = pool + (J.dst + r) * (int64_t)F;
        copy_row<V2>(d, s, F, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// submaps from a whole map, radius mode ([REF roman/map/map.py:297-339]): which segments of the map belong to
// each submap, in which order, and their feature rows in the submap's gravity-aligned frame — the feature pool the batch
// calls consume, in fixed slots of `cap` rows per submap.
//   k_submap_points   the N centres out of the N x F segment table into a dense N x 3 array: every submap's sweep then reads
//                     centres (and the N x 2 times) coalesced instead of one 24-byte piece per F-double row;
//   k_submap_select   one workgroup per submap sweeps the N segments: the radius and the time-window test, the survivors
//                     compacted in map order into a candidate list of (key, map index) with a ballot plus the counts of the
//                     waves in front (k_shared_mark's idiom: no atomics).  The first SUBMAP_LDS_CAND candidates live in LDS
//                     (48 KB), the others in the submap's slice of a global scratch the context owns: none is dropped.  With
//                     max_size set, a candidate's output position is its rank under (key, map index) — Python's stable
//                     sorted() over the list in map order [REF :332-339] — counted with uniform (broadcast) reads of the list;
//                     ranks are a permutation, so order needs no atomics either.  A NaN key sorts as +inf;
//   k_submap_gather   a wave per selected row: the centre through T_center_odom, each component ((r0 x + r1 y) + r2 z) + t,
//                     the other columns bit for bit as 64-bit words — 16 bytes per lane where source and destination of the
//                     row's tail share their 16-byte phase (one leading word peeled when both are odd), 8 otherwise;
//   k_submap_desc     mean_semantic [REF :343-346]: a thread per descriptor column adds the rows in output order.
// ---------------------------------------------------------------------------------------------
constexpr int SUBMAP_NT = 256;
constexpr int SUBMAP_LDS_CAND = 4096;                            // candidates of a submap held in LDS (8 + 4 bytes each)

// ONE kernel set serves every form: a single map is a session of one map.  The R segment tables
// lie concatenated in map order, and the HOST stages one record per LAUNCHED submap — its centre, the first segment row of its map, the
// map's rows, the start of its spill slice, its output slot —: one uniform load, no search, and the spill offset (a prefix over
// S_r * max(N_r - SUBMAP_LDS_CAND, 0)) has no closed form a workgroup could compute anyway.  Everything a workgroup does for its
// submap runs over ITS map's rows only: src holds map-local indices.
struct SubmapJob {
    roman_submap_desc_t D;   // the centre as the caller prepared it
    int64_t seg0;            // first row of the submap's map in the concatenated tables (seg_off[r]; 0 for a single map)
    int64_t spill0;          // first entry of the submap's slice of the spill
    int32_t N;               // rows of the map (seg_off[r + 1] - seg_off[r])
    int32_t slot;            // the global submap index g the record serves: its place in every output (the list forms read it: their grid runs
                             // over the listed submaps, not over the slots; everywhere else job b serves slot b)
};

// centre i of a table of F-double rows into the dense array
__device__ __forceinline__ void submap_point_one(int64_t i, int F, const double* __restrict__ feats, double* __restrict__ pts)
{
    const double* r = feats + i * (int64_t)F;
    pts[3 * i] = r[0]; pts[3 * i + 1] = r[1]; pts[3 * i + 2] = r[2];
}

__global__ void __launch_bounds__(256) k_submap_points(int64_t N, int F, const double* __restrict__ feats, double* __restrict__ pts)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    submap_point_one(i, F, feats, pts);
}

// The workgroup's work for ONE submap: `D` its centre, `pts` / `times` the N centres and times of ITS map (indices 0 .. N - 1 are what
// src receives), gKey / gIdx its slice of the spill, count / status its two words, `out` its slot of `cap` indices.
__device__ __forceinline__ void submap_select_one(const roman_submap_params_t& P, const roman_submap_desc_t& D, int N,
                                                  const double* __restrict__ pts, const double* __restrict__ times,
                                                  double* gKey, int32_t* gIdx,       // candidates SUBMAP_LDS_CAND, SUBMAP_LDS_CAND + 1, ... of this submap
                                                  int32_t* __restrict__ count, int32_t* __restrict__ out, int32_t* __restrict__ status)
{
    __shared__ double keyL[SUBMAP_LDS_CAND];
    __shared__ int32_t idxL[SUBMAP_LDS_CAND];
    __shared__ int wcnt[SUBMAP_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const bool ordered = P.max_size > 0;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += SUBMAP_NT) {                   // (uniform bounds: every barrier below is met by the whole workgroup)
        const int i = i0 + tid;
        bool member = i < N;
        double key = 0.0;
        if (member) {
            const double x = pts[3 * (int64_t)i], y = pts[3 * (int64_t)i + 1], z = pts[3 * (int64_t)i + 2];
            const double first = times[2 * (int64_t)i], last = times[2 * (int64_t)i + 1];
            if (P.use_radius) {
                const double dx = x - D.pos[0], dy = y - D.pos[1], dz = z - D.pos[2];
                member = sqrt((dx * dx + dy * dy) + dz * dz) < P.radius;
            }
            member = member && !(first > D.t_hi || last < D.t_lo);
            if (member && ordered) {
                if (P.prune_by_time) key = fabs((first + last) / 2.0 - D.time);
                else {
                    const double* T = D.T_center_odom;
                    const double cx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
                    const double cy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
                    const double cz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
                    key = sqrt((cx * cx + cy * cy) + cz * cz);
                }
                if (!(key == key)) key = INFINITY;
            }
        }
        const unsigned long long m = __ballot(member);
        __syncthreads();                                         // the counts of the previous chunk have been read
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SUBMAP_NT / 64; ++w) { const int cw = wcnt[w]; before += (w < wave) ? cw : 0; total += cw; }
        if (member) {
            const int p = base + before + __popcll(m & lt);
            if (p < SUBMAP_LDS_CAND) { keyL[p] = key; idxL[p] = i; }
            else { gKey[p - SUBMAP_LDS_CAND] = key; gIdx[p - SUBMAP_LDS_CAND] = i; }
        }
        base += total;
    }
    __syncthreads();                                             // the list is complete (LDS and, at workgroup scope, the spill)
    const int n = base, outN = min(n, P.cap), nL = min(n, SUBMAP_LDS_CAND);
    if (tid == 0) { *count = outN; *status = (!ordered && n > P.cap) ? ROMAN_ST_ASSOC_TRUNCATED : ROMAN_ST_OK; }
    if (!ordered) {                                              // map order: the list as it stands
        for (int i = tid; i < outN; i += SUBMAP_NT) out[i] = i < SUBMAP_LDS_CAND ? idxL[i] : gIdx[i - SUBMAP_LDS_CAND];
        return;
    }
    for (int i = tid; i < n; i += SUBMAP_NT) {
        const double ki = i < SUBMAP_LDS_CAND ? keyL[i] : gKey[i - SUBMAP_LDS_CAND];
        const int32_t ii = i < SUBMAP_LDS_CAND ? idxL[i] : gIdx[i - SUBMAP_LDS_CAND];
        int r = 0;
#pragma unroll 4
        for (int j = 0; j < nL; ++j) { const double kj = keyL[j]; r += (kj < ki || (kj == ki && idxL[j] < ii)) ? 1 : 0; }
        for (int j = SUBMAP_LDS_CAND; j < n; ++j) { const double kj = gKey[j - SUBMAP_LDS_CAND]; r += (kj < ki || (kj == ki && gIdx[j - SUBMAP_LDS_CAND] < ii)) ? 1 : 0; }
        if (r < outN) out[r] = ii;
    }
}

// Workgroup b serves job b and writes count[b], src[b * cap ..] and status[b]: the caller's arrays where job b is slot b, a scratch of
// the context in the list forms, whose k_submap_store_list then writes slot jobs[b].slot from there.
__global__ void __launch_bounds__(SUBMAP_NT) k_submap_select(roman_submap_params_t P, int n, const SubmapJob* __restrict__ jobs,
                                                             const double* __restrict__ pts, const double* __restrict__ times,
                                                             double* spillKey, int32_t* spillIdx,
                                                             int32_t* __restrict__ count, int32_t* __restrict__ src, int32_t* __restrict__ status)
{
    const int b = blockIdx.x;
    if (b >= n) return;
    const SubmapJob J = jobs[b];                                 // (uniform: the whole workgroup serves one submap of one map)
    submap_select_one(P, J.D, J.N, pts + 3 * J.seg0, times + 2 * J.seg0, spillKey + J.spill0, spillIdx + J.spill0,
                      count + b, src + (int64_t)b * P.cap, status + b);
}

// One word (or 16-byte pair) of an output slot.  CMP (the list forms): the OLD value is read before the new one is
// stored and `diff` learns whether a bit of it changes; without CMP this is the plain store it replaces.
__device__ __forceinline__ bool slot_differs(const ulonglong2 a, const ulonglong2 b) { return a.x != b.x || a.y != b.y; }
template <typename T> __device__ __forceinline__ bool slot_differs(const T a, const T b) { return a != b; }
template <bool CMP, typename T> __device__ __forceinline__ void slot_put(T* p, const T v, bool& diff)
{
    if constexpr (CMP) { const T was = *p; diff = diff || slot_differs(was, v); }
    *p = v;
}

// The wave's work for ONE selected row: segment k of the table `feats` (its id in `ids`) into pool row `row`, its centre through T.
// -> CMP: whether a bit of the row (or of its id) changed, per lane; otherwise false.
template <bool CMP = false>
__device__ __forceinline__ bool submap_gather_row(int point_dim, int F, const double* __restrict__ T, const unsigned long long* __restrict__ feats,
                                                  const int64_t* __restrict__ ids, int k, int64_t row,
                                                  unsigned long long* __restrict__ pool, int64_t* __restrict__ ids_out, int lane)
{
    const int Fo = point_dim + F - 3, rest = F - 3;
    const unsigned long long* in = feats + (int64_t)k * F;
    unsigned long long* out = pool + row * Fo;
    bool diff = false;
    if (lane == 0) {
        const double x = __longlong_as_double((long long)in[0]), y = __longlong_as_double((long long)in[1]), z = __longlong_as_double((long long)in[2]);
        for (int c = 0; c < point_dim; ++c)
            slot_put<CMP>(out + c, (unsigned long long)__double_as_longlong(((T[4 * c] * x + T[4 * c + 1] * y) + T[4 * c + 2] * z) + T[4 * c + 3]), diff);
        if (ids_out) slot_put<CMP>(ids_out + row, ids[k], diff);
    }
    const unsigned long long* a = in + 3;
    unsigned long long* b = out + point_dim;
    const unsigned oa = (unsigned)(((uintptr_t)a >> 3) & 1u), ob = (unsigned)(((uintptr_t)b >> 3) & 1u);
    if (oa == ob) {                                              // one 16-byte phase: a leading word when odd, pairs, a trailing word
        const int head = min((int)oa, rest), pairs = (rest - head) >> 1;
        if (lane == 0 && head) slot_put<CMP>(b, a[0], diff);
        const ulonglong2* a2 = reinterpret_cast<const ulonglong2*>(a + head);
        ulonglong2* b2 = reinterpret_cast<ulonglong2*>(b + head);
        for (int q = lane; q < pairs; q += 64) slot_put<CMP>(b2 + q, a2[q], diff);
        if (lane == 63 && head + 2 * pairs < rest) slot_put<CMP>(b + rest - 1, a[rest - 1], diff);
    } else {
        for (int q = lane; q < rest; q += 64) slot_put<CMP>(b + q, a[q], diff);
    }
    return diff;
}

// grid (submaps of all maps, row groups); a wave per selected row.  The 16-byte phase is read off the addresses in submap_gather_row:
// a map's first row sits at seg0 * F * 8 bytes, 8 mod 16 for odd seg0 * F.
__global__ void __launch_bounds__(256) k_submap_gather(int point_dim, int cap, int F, const SubmapJob* __restrict__ jobs,
                                                       const unsigned long long* __restrict__ feats, const int64_t* __restrict__ ids,
                                                       const int32_t* __restrict__ count, const int32_t* __restrict__ src,
                                                       unsigned long long* __restrict__ pool, int64_t* __restrict__ ids_out)
{
    const int g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = count[g];
    const int64_t seg0 = jobs[g].seg0;
    const unsigned long long* mfeats = feats + seg0 * F;
    const int64_t* mids = ids ? ids + seg0 : nullptr;
    for (int r = blockIdx.y * 4 + wave; r < n; r += 4 * gridDim.y) {
        const int64_t row = (int64_t)g * cap + r;
        submap_gather_row(point_dim, F, jobs[g].D.T_center_odom, mfeats, mids, src[row], row, pool, ids_out, lane);
    }
}

// column c of ONE submap's mean_semantic descriptor: the n rows `rows` names of the table `feats`, added in output order
__device__ __forceinline__ double submap_desc_col(int F, int d, int c, const double* __restrict__ feats, const int32_t* __restrict__ rows, int n)
{
    double acc = 0.0;
    for (int r = 0; r < n; ++r) acc += feats[(int64_t)rows[r] * F + (F - d) + c];
    return acc / (double)n;
}

__device__ __forceinline__ void submap_desc_one(int F, int d, int c, const double* __restrict__ feats, const int32_t* __restrict__ rows, int n,
                                                double* __restrict__ desc)
{
    desc[c] = submap_desc_col(F, d, c, feats, rows, n);
}

// grid (submaps of all maps, column groups): desc_out[g][c] = (sum over the rows of submap g, in output order, of descriptor column c) / count
__global__ void __launch_bounds__(256) k_submap_desc(int cap, int F, int d, const SubmapJob* __restrict__ jobs, const double* __restrict__ feats,
                                                     const int32_t* __restrict__ count, const int32_t* __restrict__ src, double* __restrict__ desc_out)
{
    const int g = blockIdx.x, c = blockIdx.y * blockDim.x + threadIdx.x;
    const int n = count[g];
    if (c >= d || n == 0) return;                                // an empty submap's descriptor is left as it was
    submap_desc_one(F, d, c, feats + jobs[g].seg0 * F, src + (int64_t)g * cap, n, desc_out + (int64_t)g * d);
}

// The LIST forms (roman_session_submaps_list*): only the L listed submaps of the session are rebuilt, each WHOLE —
// a submap may shrink —, and the call reports which slots changed.  `jobs` holds the L LISTED submaps' records (jobs[l].slot is the
// global index g), the grids run over L.  k_submap_select writes count, status and the ordered indices of listed submap l into a
// scratch of the context (newCount[l], newStatus[l], newSrc[l * cap ..]); the store kernel then writes slot g from there.  The dense
// centres come from k_submap_points over the maps that have a listed submap.
// The wave's work for ONE row of a listed slot beyond its count: the values the Python layer clears its tensors to (pool 0.0, id -1),
// with submap_gather_row's 16-byte phase logic on the destination: a leading word when the row starts odd, pairs, a trailing word.
template <bool CMP>
__device__ __forceinline__ bool submap_clear_row(int Fo, int64_t row, unsigned long long* __restrict__ pool, int64_t* __restrict__ ids_out, int lane)
{
    unsigned long long* b = pool + row * Fo;
    bool diff = false;
    if (lane == 0 && ids_out) slot_put<CMP>(ids_out + row, (int64_t)-1, diff);
    const unsigned ob = (unsigned)(((uintptr_t)b >> 3) & 1u);
    const int head = min((int)ob, Fo), pairs = (Fo - head) >> 1;
    if (lane == 0 && head) slot_put<CMP>(b, 0ull, diff);
    ulonglong2* b2 = reinterpret_cast<ulonglong2*>(b + head);
    for (int q = lane; q < pairs; q += 64) slot_put<CMP>(b2 + q, make_ulonglong2(0ull, 0ull), diff);
    if (lane == 63 && head + 2 * pairs < Fo) slot_put<CMP>(b + Fo - 1, 0ull, diff);
    return diff;
}

// One workgroup per listed submap writes its WHOLE slot: count and status, the `cap` indices of src (-1 beyond the count), the rows
// [0, count) through submap_gather_row (a wave per row), the rows [count, cap) through submap_clear_row, and the mean_semantic row
// through submap_desc_col (all NaN for an empty submap) — every byte by exactly one thread, which with CMP reads the old value right
// before it stores the new one.  changed[l]: whether any thread saw a difference — one __syncthreads_or and one plain store, so the
// flag does not depend on any order.  Nothing of an unlisted slot is read or written.
template <bool CMP>
__global__ void __launch_bounds__(256) k_submap_store_list(int point_dim, int cap, int F, int d, const SubmapJob* __restrict__ jobs,
                                                           const unsigned long long* __restrict__ feats, const int64_t* __restrict__ ids,
                                                           const int32_t* __restrict__ newCount, const int32_t* __restrict__ newSrc,
                                                           const int32_t* __restrict__ newStatus,
                                                           unsigned long long* __restrict__ pool, int32_t* __restrict__ count, int32_t* __restrict__ src,
                                                           int64_t* __restrict__ ids_out, int32_t* __restrict__ status,
                                                           unsigned long long* __restrict__ desc_out, int32_t* __restrict__ changed)
{
    const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg0 = jobs[l].seg0;                           // (uniform)
    const int g = jobs[l].slot, n = newCount[l];
    const int32_t* rows = newSrc + (int64_t)l * cap;
    const unsigned long long* mfeats = feats + seg0 * F;
    const int64_t* mids = ids ? ids + seg0 : nullptr;
    bool diff = false;
    if (tid == 0) { slot_put<CMP>(count + g, (int32_t)n, diff); slot_put<CMP>(status + g, newStatus[l], diff); }
    for (int i = tid; i < cap; i += 256) slot_put<CMP>(src + (int64_t)g * cap + i, i < n ? rows[i] : (int32_t)-1, diff);
    for (int r = wave; r < cap; r += 4) {                        // (r is uniform over the wave)
        const int64_t row = (int64_t)g * cap + r;
        const bool x = r < n ? submap_gather_row<CMP>(point_dim, F, jobs[l].D.T_center_odom, mfeats, mids, rows[r], row, pool, ids_out, lane)
                             : submap_clear_row<CMP>(point_dim + F - 3, row, pool, ids_out, lane);
        diff = diff || x;
    }
    if (desc_out)
        for (int c = tid; c < d; c += 256) {
            const unsigned long long v = n ? (unsigned long long)__double_as_longlong(submap_desc_col(F, d, c, reinterpret_cast<const double*>(mfeats), rows, n))
                                           : 0x7ff8000000000000ull;                  // the quiet NaN the Python layer fills its descriptors with
            slot_put<CMP>(desc_out + (int64_t)g * d + c, v, diff);
        }
    if constexpr (CMP) {
        const int any = __syncthreads_or(diff ? 1 : 0);
        if (tid == 0) changed[l] = any ? 1 : 0;
    }
}

// Submap.segments_as_global_points [REF roman/map/map.py:133-139] reduced to what aabb_intersects [REF roman/utils.py:160-169] reads
// of it: ONE WAVE per submap takes rows [s * cap, s * cap + count[s]) of the pool to the global frame with the submap's
// T_odom_center — each component ((r0 x + r1 y) + r2 z) + t, k_submap_gather's arithmetic — and reduces them to
// box[s] = (min x, min y, min z, max x, max y, max z).  Rows beyond 64 are taken in further steps of the same wave; min and max of
// finite doubles are exact and order-free, so the butterfly's order is free.  An empty submap: (+inf x 3, -inf x 3), never nearby.
// (the wave's work in k_submap_boxes and k_session_boxes: `rows` the submap's first row, `n` its rows, `T` its pose, `out` its box)
__device__ __forceinline__ void box_of_rows(const double* __restrict__ rows, int n, int F, const double* __restrict__ T, double* __restrict__ out, int lane)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = lane; r < n; r += 64) {
        const double* p = rows + (int64_t)r * F;
        const double x = p[0], y = p[1], z = p[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = ((T[4 * c] * x + T[4 * c + 1] * y) + T[4 * c + 2] * z) + T[4 * c + 3];
            lo[c] = fmin(lo[c], v); hi[c] = fmax(hi[c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { lo[c] = fmin(lo[c], __shfl_xor(lo[c], off)); hi[c] = fmax(hi[c], __shfl_xor(hi[c], off)); }
    if (lane < 3) {
        const double l = lane == 0 ? lo[0] : (lane == 1 ? lo[1] : lo[2]), h = lane == 0 ? hi[0] : (lane == 1 ? hi[1] : hi[2]);
        out[lane] = l; out[3 + lane] = h;
    }
}

__global__ void __launch_bounds__(256) k_submap_boxes(int S, int F, int cap, const double* __restrict__ pool, const int32_t* __restrict__ count,
                                                      const double* __restrict__ T_odom_center, double* __restrict__ box)
{
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;                                          // (wave-uniform)
    const int n = max(0, min(count[s], cap));                    // (a count outside its slot reads nothing beyond it)
    box_of_rows(pool + (int64_t)s * cap * F, n, F, T_odom_center + 16 * (int64_t)s, box + 6 * (int64_t)s, lane);
}

// The same over the submap table of a SESSION (roman_session_boxes*): one wave per global submap g — a submap of a
// view (§4.14) — whose rows are [row0[g], row0[g] + count[g]) of the ONE concatenated pool the batch reads anyway: no launch per
// robot, no gather of the rows into slots.  Two views of one robot name the same rows with their own T_odom_center; everything but
// `box` is read-only.  Latency-bound (one strided row read per lane: three columns of a row of F doubles); not measured at session
// scale beyond DESIGN.md §6.16.
__global__ void __launch_bounds__(256) k_session_boxes(int S, int F, const double* __restrict__ pool, const int64_t* __restrict__ row0,
                                                       const int32_t* __restrict__ count, const double* __restrict__ T_odom_center, double* __restrict__ box)
{
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= S) return;                                          // (wave-uniform)
    box_of_rows(pool + row0[g] * F, max(0, count[g]), F, T_odom_center + 16 * (int64_t)g, box + 6 * (int64_t)g, lane);
}

// ---------------------------------------------------------------------------------------------
// pass 1 of the pair loop for a whole S0 x S1 grid ([REF roman/align/submap_align.py:93-149], radius mode):
// distance and radius gate, reference transform, yaw difference, submap-descriptor similarity, the skip / gated / todo
// classes, and the TODO pairs compacted in row-major order with their reference transform and time-gate flag — what
// roman_align_lc_batch_dev / roman_lc_tail_dev read.
//   k_grid_norms    a wave per submap (both sides): the descriptor's norm, once per submap instead of once per pair;
//   k_grid_gate     a wave per (i, GRID_TJ consecutive j): lane l walks components l, l + 64, ... of descriptor i ONCE against
//                   GRID_TJ descriptors of the other side (coalesced 512-byte row pieces, GRID_TJ independent sums), a butterfly
//                   adds the 64 partial sums — a fixed order, no atomics: two runs agree bit for bit —, then lane t finishes pair
//                   (i, j0 + t): a few dozen f64 operations and the dense outputs.  With AABB (roman_grid_gate_aabb*, DESIGN.md
//                   §4.12) NEARBY is the six comparisons of aabb_intersects [REF roman/utils.py:167-169] on the two submaps'
//                   boxes (k_submap_boxes) instead of dist < 2 * radius; nothing else changes;
//   k_grid_compact  one workgroup: the TODO pairs in row-major order through block_excl_scan (k_lc_compact's idiom);
//   k_grid_fill     16 threads per compact slot: T_ref <- T_ij of the slot's pair, bit for bit, and the time gate
//                   [REF roman/align/results.py:160-162].  Slots beyond n_todo are not written.
// ---------------------------------------------------------------------------------------------
constexpr int GRID_TJ = 4;                                       // pairs of one row a wave of k_grid_gate handles
constexpr int GRID_NEARBY = 1, GRID_SKIP = 2, GRID_GATED = 4, GRID_TODO = 8;    // ROMAN_GRID_* of roman_hip.h

struct GridSide { const double* pos; const double* pos_gt; const double* T_w; const double* time; const double* desc; const double* box; };
struct GridOut { double* dist; int32_t* flags; double* yaw_deg; double* sim; double* T_ij; };

// sum over the 64 lanes, the same bits in every lane (x + y == y + x)
__device__ __forceinline__ double wave_sum_all(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(256) k_grid_norms(int S0, int S1, int d, const double* __restrict__ desc0, const double* __restrict__ desc1,
                                                    double* __restrict__ norm)
{
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= S0 + S1) return;                                    // (wave-uniform)
    const double* v = w < S0 ? desc0 + (int64_t)w * d : desc1 + (int64_t)(w - S0) * d;
    double s = 0.0;
    for (int k = lane; k < d; k += 64) { const double x = v[k]; s += x * x; }
    s = wave_sum_all(s);
    if (lane == 0) norm[w] = sqrt(s);
}

// One pair of pass 1 — what k_grid_gate and k_session_gate do once the descriptors' dot product is known: submap i of side a against
// submap j of side b (indices into the sides' arrays), `gt`: the distance is between the ground-truth centres, `np_`: the product of the
// two descriptor norms (read with d > 0 only), `p`: the pair's place in the dense outputs.
template <bool SIM_IN, bool AABB>
__device__ __forceinline__ void grid_pair(const roman_grid_gate_params_t& P, const GridSide& a, const GridSide& b, int64_t i, int64_t j, bool gt, int d,
                                          double dot, double np_, int64_t p, const GridOut& out)
{
    const double* pa = (gt ? a.pos_gt : a.pos) + 3 * i;
    const double* pb = (gt ? b.pos_gt : b.pos) + 3 * j;
    const double dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
    bool nearby;
    if (AABB) {                                                  // <= and >= as they stand: touching boxes intersect [REF roman/utils.py:167-169]
        const double* A = a.box + 6 * i;
        const double* Bx = b.box + 6 * j;
        nearby = A[0] <= Bx[3] && A[3] >= Bx[0] && A[1] <= Bx[4] && A[4] >= Bx[1] && A[2] <= Bx[5] && A[5] >= Bx[2];
    } else nearby = dist < 2.0 * P.radius;
    double Ti[16], T[16];
    lc_inv_affine(a.T_w + 16 * i, Ti);
    lc_mul4(Ti, b.T_w + 16 * j, T);
    const double yaw = nearby ? fabs(atan2(T[4], T[0]) * (180.0 / 3.141592653589793)) : d_nan();    // |np.rad2deg(yaw)|
    double sim = INFINITY;
    if (SIM_IN) sim = out.sim[p];
    else if (d > 0) sim = (np_ <= 1e-9) ? 0.0 : dot / np_;       // np.isclose(norm_prod, 0, atol=1e-9, rtol=0) [REF roman/map/map.py:151-153]
    const bool skip = dist > P.skip_distance;                    // [REF :136]
    const bool gated = !skip && sim < P.desc_thresh;
    const bool todo = !skip && !gated;
    out.dist[p] = dist; out.yaw_deg[p] = yaw;
    if (!SIM_IN) out.sim[p] = sim;
    out.flags[p] = (nearby ? GRID_NEARBY : 0) | (skip ? GRID_SKIP : 0) | (gated ? GRID_GATED : 0) | (todo ? GRID_TODO : 0);
    double* To = out.T_ij + 16 * p;
#pragma unroll
    for (int t = 0; t < 16; ++t) To[t] = T[t];
}

// SIM_IN (roman_grid_gate_sim*): the similarity of every pair is already in out.sim — read, never written — and no descriptor is touched
// AABB (roman_grid_gate_aabb*): NEARBY from a.box[i] and b.box[j] (float64[6]: min x y z, max x y z), P.radius is not read
template <bool SIM_IN, bool AABB>
__global__ void __launch_bounds__(256) k_grid_gate(roman_grid_gate_params_t P, int S0, int S1, GridSide a, GridSide b,
                                                   const double* __restrict__ norm, GridOut out)
{
    const int lane = threadIdx.x & 63;
    const int nT = (S1 + GRID_TJ - 1) / GRID_TJ;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (int64_t)S0 * nT) return;                           // (wave-uniform)
    const int i = (int)(w / nT), j0 = (int)(w % nT) * GRID_TJ;
    const int d = SIM_IN ? 0 : P.desc_dim;
    double acc[GRID_TJ];
#pragma unroll
    for (int t = 0; t < GRID_TJ; ++t) acc[t] = 0.0;
    if (d > 0) {
        const double* va = a.desc + (int64_t)i * d;
        const double* vb[GRID_TJ];
#pragma unroll
        for (int t = 0; t < GRID_TJ; ++t) vb[t] = b.desc + (int64_t)min(j0 + t, S1 - 1) * d;    // (a tile's tail repeats the last row: in bounds, never stored)
        for (int k = lane; k < d; k += 64) {
            const double x = va[k];
#pragma unroll
            for (int t = 0; t < GRID_TJ; ++t) acc[t] += x * vb[t][k];
        }
#pragma unroll
        for (int t = 0; t < GRID_TJ; ++t) acc[t] = wave_sum_all(acc[t]);
    }
    const int j = j0 + lane;
    if (lane >= GRID_TJ || j >= S1) return;
    double dot = acc[0];
#pragma unroll
    for (int t = 1; t < GRID_TJ; ++t) dot = (lane == t) ? acc[t] : dot;
    const double np_ = (!SIM_IN && d > 0) ? norm[i] * norm[S0 + j] : 0.0;
    grid_pair<SIM_IN, AABB>(P, a, b, i, j, a.pos_gt != nullptr && b.pos_gt != nullptr /* [REF :96-99] */, d, dot, np_, (int64_t)i * S1 + j, out);
}

__global__ void __launch_bounds__(1024) k_grid_compact(int B, int S1, const int32_t* __restrict__ flags, int32_t* __restrict__ pairs, int32_t* __restrict__ n_todo)
{
    __shared__ int shi[17];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int PER = (B + nt - 1) / nt;
    const int b0 = min(B, tid * PER), b1 = min(B, b0 + PER);
    int mine = 0;
    for (int b = b0; b < b1; ++b) mine += (flags[b] & GRID_TODO) ? 1 : 0;
    int total;
    int pos = block_excl_scan(mine, shi, total);
    for (int b = b0; b < b1; ++b)
        if (flags[b] & GRID_TODO) { pairs[2 * (int64_t)pos] = b / S1; pairs[2 * (int64_t)pos + 1] = b % S1; ++pos; }
    if (tid == 0) *n_todo = total;
}

__global__ void __launch_bounds__(256) k_grid_fill(roman_grid_gate_params_t P, int S1, const int32_t* __restrict__ n_todo, const int32_t* __restrict__ pairs,
                                                   const double* __restrict__ T_ij, const double* __restrict__ time0, const double* __restrict__ time1,
                                                   double* __restrict__ T_ref, int32_t* __restrict__ enable)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = g >> 4;
    const int e = (int)(g & 15);
    if (s >= *n_todo) return;
    const int i = pairs[2 * s], j = pairs[2 * s + 1];
    T_ref[16 * s + e] = T_ij[16 * ((int64_t)i * S1 + j) + e];
    if (e == 0) enable[s] = (P.single_robot_lc && fabs(time0[i] - time1[j]) < P.lc_time_thresh) ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------
// pass 1 of a whole multi-robot session (roman_session_gate*): the grids of a LIST of robot pairs ("blocks") over
// ONE set of per-submap arrays — robot r owns the global submaps [sub_off[r], sub_off[r + 1]) —, in one launch sequence.  Block b is
// (r0, r1, self_lc, 0); its n0 x n1 grid lies row-major at pair_off[b] of the dense outputs, its tiles at tile_off[b].
//   k_grid_norms      over all S submaps (S1 = 0);
//   k_session_gate    k_grid_gate's wave — (block, row i, GRID_TJ consecutive columns), the block by a wave-uniform binary search of
//                     tile_off —, the same lane layout of the dot product and the same per-pair body (grid_pair): a block's dense
//                     values are bit for bit what k_grid_gate writes for its two sides;
//   k_session_count   the TODO flags of 1024 consecutive pairs: ballot + popcount per wave, the 16 wave counts added in LDS;
//   k_session_scan    one workgroup: the exclusive scan of the workgroup counts, 1024 at a time (block_excl_scan with a carry), and
//                     todo_off of the blocks that start at the end of the flags (trailing empty blocks, and todo_off[nb]: the total);
//   k_session_scatter recounts its 1024 flags, adds the scanned base and writes (gi, gj) of every TODO pair at its rank; the thread
//                     of a block's FIRST flag writes that block's todo_off (and that of the empty blocks in front of it);
//   k_session_fill    k_grid_fill with global indices: the block of a compact slot by binary search of todo_off, T_ref from the
//                     block's dense T_ij, enable = 0 only where the block's self_lc is set and the two times are close.
// No atomics, no spin-waits, no cooperative launch: the order of every sum is fixed, two runs agree bit for bit.
// ---------------------------------------------------------------------------------------------
constexpr int SESSION_SCAN = 1024;                               // flags per workgroup of the compaction

struct SessionTab { int nb; const int32_t* sub_off; const int32_t* blocks; const int64_t* pair_off; const int64_t* tile_off; const int32_t* has_gt; };

// the last k in [0, n) with off[k] <= x (off ascending, off[0] <= x): the block that holds x — of several that start at the same place,
// the last one, the only one that is not empty
__device__ __forceinline__ int session_find(const int64_t* __restrict__ off, int n, int64_t x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

__device__ __forceinline__ int session_find(const int32_t* __restrict__ off, int n, int64_t x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// a wave of k_session_gate — SIM_IN and AABB as grid_pair has them
template <bool SIM_IN, bool AABB>
__device__ __forceinline__ void session_gate_wave(roman_grid_gate_params_t P, SessionTab tab, int64_t tiles, GridSide s,
                                                  const double* __restrict__ norm, GridOut out)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= tiles) return;                                      // (wave-uniform, as everything up to the lanes' pairs)
    const int b = session_find(tab.tile_off, tab.nb, w);
    const int r0 = tab.blocks[4 * b], r1 = tab.blocks[4 * b + 1];
    const int base0 = tab.sub_off[r0], base1 = tab.sub_off[r1], n1 = tab.sub_off[r1 + 1] - base1;
    const int nT = (n1 + GRID_TJ - 1) / GRID_TJ;
    const int64_t lw = w - tab.tile_off[b];
    const int i = (int)(lw / nT), j0 = (int)(lw % nT) * GRID_TJ;
    const int d = SIM_IN ? 0 : P.desc_dim;
    double acc[GRID_TJ];
#pragma unroll
    for (int t = 0; t < GRID_TJ; ++t) acc[t] = 0.0;
    if (d > 0) {
        const double* va = s.desc + (int64_t)(base0 + i) * d;
        const double* vb[GRID_TJ];
#pragma unroll
        for (int t = 0; t < GRID_TJ; ++t) vb[t] = s.desc + (int64_t)(base1 + min(j0 + t, n1 - 1)) * d;    // (a tile's tail repeats the block's last row)
        for (int k = lane; k < d; k += 64) {
            const double x = va[k];
#pragma unroll
            for (int t = 0; t < GRID_TJ; ++t) acc[t] += x * vb[t][k];
        }
#pragma unroll
        for (int t = 0; t < GRID_TJ; ++t) acc[t] = wave_sum_all(acc[t]);
    }
    const int j = j0 + lane;
    if (lane >= GRID_TJ || j >= n1) return;
    double dot = acc[0];
#pragma unroll
    for (int t = 1; t < GRID_TJ; ++t) dot = (lane == t) ? acc[t] : dot;
    const int64_t gi = base0 + i, gj = base1 + j;
    const bool gt = s.pos_gt != nullptr && tab.has_gt[r0] != 0 && tab.has_gt[r1] != 0;      // [REF :96-99]
    const double np_ = (!SIM_IN && d > 0) ? norm[gi] * norm[gj] : 0.0;
    grid_pair<SIM_IN, AABB>(P, s, s, gi, gj, gt, d, dot, np_, tab.pair_off[b] + (int64_t)i * n1 + j, out);
}

// SIM_IN (roman_session_gate_sim*): the similarity of every pair is already in out.sim — read, never written — and no descriptor is touched
template <bool SIM_IN>
__global__ void __launch_bounds__(256) k_session_gate(roman_grid_gate_params_t P, SessionTab tab, int64_t tiles, GridSide s,
                                                      const double* __restrict__ norm, GridOut out)
{
    session_gate_wave<SIM_IN, false>(P, tab, tiles, s, norm, out);
}

// the second switch k_grid_gate has, as an overload: k_session_gate<SIM_IN> above keeps its name and its launches.  AABB
// (roman_session_gate_aabb*): NEARBY from s.box[gi] and s.box[gj] (k_session_boxes), P.radius is not read
template <bool SIM_IN, bool AABB>
__global__ void __launch_bounds__(256) k_session_gate(roman_grid_gate_params_t P, SessionTab tab, int64_t tiles, GridSide s,
                                                      const double* __restrict__ norm, GridOut out)
{
    session_gate_wave<SIM_IN, AABB>(P, tab, tiles, s, norm, out);
}

// the TODO flags of this workgroup's SESSION_SCAN pairs: -> (is flag g TODO, TODO flags of the workgroup in front of g, their number in the workgroup)
__device__ __forceinline__ void session_rank(const int32_t* __restrict__ flags, int64_t total, int64_t g, int* sh, bool& mine, int& rank, int& count)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    mine = g < total && (flags[g] & GRID_TODO) != 0;
    const unsigned long long m = __ballot(mine);
    if (lane == 0) sh[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < SESSION_SCAN / 64; ++k) { const int x = sh[k]; if (k < w) base += x; tot += x; }
    rank = base + __popcll(m & ((1ull << lane) - 1ull));
    count = tot;
}

__global__ void __launch_bounds__(SESSION_SCAN) k_session_count(int64_t total, const int32_t* __restrict__ flags, int32_t* __restrict__ counts)
{
    __shared__ int sh[SESSION_SCAN / 64];
    bool mine; int rank, count;
    session_rank(flags, total, (int64_t)blockIdx.x * SESSION_SCAN + threadIdx.x, sh, mine, rank, count);
    if (threadIdx.x == 0) counts[blockIdx.x] = count;
}

// counts[k] <- the TODO flags in front of workgroup k (in place) -> their total: the scan of k_session_scan and k_session_list_scan
__device__ __forceinline__ int session_scan_counts(int nwg, int32_t* __restrict__ counts, int* shi)
{
    int carry = 0;
    for (int k0 = 0; k0 < nwg; k0 += SESSION_SCAN) {             // (uniform trip count: block_excl_scan has barriers)
        const int k = k0 + (int)threadIdx.x;
        const int v = k < nwg ? counts[k] : 0;
        int tot;
        const int ex = block_excl_scan(v, shi, tot);
        if (k < nwg) counts[k] = carry + ex;
        carry += tot;
    }
    return carry;
}

// the scan; todo_off[b] <- the total for every b whose block starts at `total`
__global__ void __launch_bounds__(SESSION_SCAN) k_session_scan(int nwg, int32_t* __restrict__ counts, SessionTab tab, int64_t total, int32_t* __restrict__ todo_off)
{
    __shared__ int shi[17];
    const int carry = session_scan_counts(nwg, counts, shi);
    for (int b = threadIdx.x; b <= tab.nb; b += SESSION_SCAN)
        if (tab.pair_off[b] == total) todo_off[b] = carry;
}

__global__ void __launch_bounds__(SESSION_SCAN) k_session_scatter(int64_t total, const int32_t* __restrict__ flags, const int32_t* __restrict__ bases,
                                                                  SessionTab tab, int32_t* __restrict__ pairs, int32_t* __restrict__ todo_off)
{
    __shared__ int sh[SESSION_SCAN / 64];
    const int64_t g = (int64_t)blockIdx.x * SESSION_SCAN + threadIdx.x;
    bool mine; int rank, count;
    session_rank(flags, total, g, sh, mine, rank, count);
    if (g >= total) return;
    const int pos = bases[blockIdx.x] + rank;
    const int b = session_find(tab.pair_off, tab.nb, g);        // (g < total: the block that holds g is not empty)
    const int64_t first = tab.pair_off[b];
    if (first == g)                                              // the block's first flag: its rank is the block's todo_off, and that of
        for (int k = b; k >= 0 && tab.pair_off[k] == g; --k) todo_off[k] = pos;     // the empty blocks listed in front of it
    if (!mine) return;
    const int r0 = tab.blocks[4 * b], r1 = tab.blocks[4 * b + 1];
    const int base1 = tab.sub_off[r1], n1 = tab.sub_off[r1 + 1] - base1;
    const int64_t l = g - first;
    pairs[2 * (int64_t)pos] = tab.sub_off[r0] + (int32_t)(l / n1);
    pairs[2 * (int64_t)pos + 1] = base1 + (int32_t)(l % n1);
}

__global__ void __launch_bounds__(256) k_session_fill(roman_grid_gate_params_t P, SessionTab tab, const int32_t* __restrict__ todo_off,
                                                      const int32_t* __restrict__ pairs, const double* __restrict__ T_ij, const double* __restrict__ time,
                                                      double* __restrict__ T_ref, int32_t* __restrict__ enable)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = g >> 4;
    const int e = (int)(g & 15);
    if (s >= todo_off[tab.nb]) return;
    const int b = session_find(todo_off, tab.nb, s);
    const int r0 = tab.blocks[4 * b], r1 = tab.blocks[4 * b + 1];
    const int base1 = tab.sub_off[r1], n1 = tab.sub_off[r1 + 1] - base1;
    const int gi = pairs[2 * s], gj = pairs[2 * s + 1];
    const int64_t p = tab.pair_off[b] + (int64_t)(gi - tab.sub_off[r0]) * n1 + (gj - base1);
    T_ref[16 * s + e] = T_ij[16 * p + e];
    if (e == 0) enable[s] = (tab.blocks[4 * b + 2] && fabs(time[gi] - time[gj]) < P.lc_time_thresh) ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------
// pass 1 of a session over an explicit PAIR LIST (roman_session_gate_list*): the tables and per-submap arrays of
// roman_session_gate*, and `list` int32[L][3] — (block, block-local row i, block-local column j), strictly ascending.  The outputs
// are per LIST ENTRY (L of each), entry l bit for bit what k_session_gate writes at pair_off[b] + i * n1 + j.
//   k_grid_norms           over all S submaps, as for the whole grids;
//   k_session_gate_list    a wave per GRID_TJ consecutive list entries.  The entries may lie in different rows and blocks, so
//                          nothing of a row is shared across them: each sum walks its own two descriptors, lane l the components
//                          l, l + 64, ... in k_session_gate's order, and wave_sum_all adds the 64 partial sums — the bits of the
//                          whole-grid kernels.  The entries are read through wave-uniform (scalar) loads; lane t then finishes
//                          entry 4 w + t through grid_pair() with the entry's index as its place in the outputs.  With SIM_IN the
//                          similarity is read at the pair's DENSE position of sim_in and copied to sim[l];
//   k_session_count        the TODO flags of 1024 consecutive entries, as it stands;
//   k_session_list_scan    k_session_scan with the blocks behind the last listed one in place of those that start at `total`;
//   k_session_list_scatter recounts, writes (gi, gj) of every TODO entry at its rank and its entry index into `src`; the thread of
//                          the first entry of a block writes that block's todo_off and that of the blocks without an entry in
//                          front of it — the block of an entry is list[l][0], no search;
//   k_session_list_fill    k_session_fill with the source entry from `src` instead of the dense position.
// No atomics, no spin-waits, no cooperative launch: two runs agree bit for bit.
// ---------------------------------------------------------------------------------------------
template <bool SIM_IN, bool AABB>
__global__ void __launch_bounds__(256) k_session_gate_list(roman_grid_gate_params_t P, SessionTab tab, int L, const int32_t* __restrict__ list,
                                                           GridSide s, const double* __restrict__ norm, const double* __restrict__ sim_in, GridOut out)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t l0 = w * GRID_TJ;
    if (l0 >= L) return;                                         // (wave-uniform, as everything up to the lanes' entries)
    const int d = SIM_IN ? 0 : P.desc_dim;
    double acc[GRID_TJ];
#pragma unroll
    for (int t = 0; t < GRID_TJ; ++t) acc[t] = 0.0;
    if (d > 0) {
        const double* va[GRID_TJ];
        const double* vb[GRID_TJ];
#pragma unroll
        for (int t = 0; t < GRID_TJ; ++t) {                      // (the last wave's tail repeats the last entry: in bounds, never stored)
            const int32_t* e = list + 3 * min(l0 + t, (int64_t)L - 1);
            const int b = e[0];
            va[t] = s.desc + (int64_t)(tab.sub_off[tab.blocks[4 * b]] + e[1]) * d;
            vb[t] = s.desc + (int64_t)(tab.sub_off[tab.blocks[4 * b + 1]] + e[2]) * d;
        }
        for (int k = lane; k < d; k += 64) {
#pragma unroll
            for (int t = 0; t < GRID_TJ; ++t) acc[t] += va[t][k] * vb[t][k];
        }
#pragma unroll
        for (int t = 0; t < GRID_TJ; ++t) acc[t] = wave_sum_all(acc[t]);
    }
    const int64_t l = l0 + lane;
    if (lane >= GRID_TJ || l >= L) return;
    double dot = acc[0];
#pragma unroll
    for (int t = 1; t < GRID_TJ; ++t) dot = (lane == t) ? acc[t] : dot;
    const int b = list[3 * l], i = list[3 * l + 1], j = list[3 * l + 2];
    const int r0 = tab.blocks[4 * b], r1 = tab.blocks[4 * b + 1];
    const int base1 = tab.sub_off[r1], n1 = tab.sub_off[r1 + 1] - base1;
    const int64_t gi = tab.sub_off[r0] + i, gj = base1 + j;
    const bool gt = s.pos_gt != nullptr && tab.has_gt[r0] != 0 && tab.has_gt[r1] != 0;      // [REF :96-99]
    const double np_ = (!SIM_IN && d > 0) ? norm[gi] * norm[gj] : 0.0;
    GridOut o = out;
    if (SIM_IN) {                                                // grid_pair reads o.sim[l]: the pair's dense similarity, and sim[l] gets its copy
        const double* at = sim_in + (tab.pair_off[b] + (int64_t)i * n1 + j);
        out.sim[l] = *at;
        o.sim = const_cast<double*>(at) - l;
    }
    grid_pair<SIM_IN, AABB>(P, s, s, gi, gj, gt, d, dot, np_, l, o);
}

// todo_off[b] <- the total for every block behind the last listed one, and for nb
__global__ void __launch_bounds__(SESSION_SCAN) k_session_list_scan(int nwg, int32_t* __restrict__ counts, int nb, int L, const int32_t* __restrict__ list,
                                                                    int32_t* __restrict__ todo_off)
{
    __shared__ int shi[17];
    const int carry = session_scan_counts(nwg, counts, shi);
    for (int b = list[3 * ((int64_t)L - 1)] + 1 + (int)threadIdx.x; b <= nb; b += SESSION_SCAN) todo_off[b] = carry;
}

__global__ void __launch_bounds__(SESSION_SCAN) k_session_list_scatter(int L, const int32_t* __restrict__ flags, const int32_t* __restrict__ bases, SessionTab tab,
                                                                       const int32_t* __restrict__ list, int32_t* __restrict__ pairs, int32_t* __restrict__ src,
                                                                       int32_t* __restrict__ todo_off)
{
    __shared__ int sh[SESSION_SCAN / 64];
    const int64_t l = (int64_t)blockIdx.x * SESSION_SCAN + threadIdx.x;
    bool mine; int rank, count;
    session_rank(flags, L, l, sh, mine, rank, count);
    if (l >= L) return;
    const int pos = bases[blockIdx.x] + rank;
    const int b = list[3 * l], before = l > 0 ? list[3 * (l - 1)] : -1;
    for (int k = b; k > before; --k) todo_off[k] = pos;         // the block's first entry: its rank is the block's todo_off, and that of
    if (!mine) return;                                           // the blocks without an entry in front of it
    pairs[2 * (int64_t)pos] = tab.sub_off[tab.blocks[4 * b]] + list[3 * l + 1];
    pairs[2 * (int64_t)pos + 1] = tab.sub_off[tab.blocks[4 * b + 1]] + list[3 * l + 2];
    src[pos] = (int32_t)l;
}

__global__ void __launch_bounds__(256) k_session_list_fill(roman_grid_gate_params_t P, SessionTab tab, const int32_t* __restrict__ todo_off,
                                                           const int32_t* __restrict__ pairs, const int32_t* __restrict__ src, const int32_t* __restrict__ list,
                                                           const double* __restrict__ T_ij, const double* __restrict__ time,
                                                           double* __restrict__ T_ref, int32_t* __restrict__ enable)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = g >> 4;
    const int e = (int)(g & 15);
    if (s >= todo_off[tab.nb]) return;
    const int64_t l = src[s];
    T_ref[16 * s + e] = T_ij[16 * l + e];
    if (e == 0) {
        const int gi = pairs[2 * s], gj = pairs[2 * s + 1];
        enable[s] = (tab.blocks[4 * list[3 * l] + 2] && fabs(time[gi] - time[gj]) < P.lc_time_thresh) ? 0 : 1;
    }
}

// ---------------------------------------------------------------------------------------------
// Frame-descriptor submaps ([REF roman/map/map.py:210-242], [REF :155-162]): which frames of a map every submap of
// a pool holds, their mean, and the stacked similarity of a whole grid from the two maps' frame tables.
//   k_frame_select   ONE WAVE per submap.  The span (min first_seen, max last_seen over the rows the submap keeps) by a lane-strided
//                    sweep and a butterfly; then the frames in words of 64: the candidate test (lo <= t <= hi) in every lane, a
//                    ballot is the mask word.  Thinning walks the set bits of the word in ascending order — a wave-uniform loop;
//                    the candidate's position comes from its lane by a shuffle, the last selected position is carried in
//                    (uniform) registers across words.  Distance sqrt((dx^2 + dy^2) + dz^2), no fused multiply-adds;
//   k_frame_mean     a thread per descriptor column adds the selected rows in ascending frame index (k_submap_desc's idiom);
//   k_stacked_band   a wave per 32 x 32 tile of the frame-cosine matrix of one row BAND of map 0 against all frames of map 1:
//                    2 x 2 blocks of v_mfma_f64_16x16x4, operands straight from global memory with 32-byte loads, k_cos's
//                    contraction order (chunks of 16 ascending, step t contracts k = k0 + 4 * (lane >> 4) + t); the epilogue
//                    divides by the norms (k_grid_norms, once per frame) with the reference's zero guard;
//   k_stacked_colmax R[i][b] = max(R[i][b], max over the band's frames a in mask0[i] of c(a, b)): a thread per (i, b) owns its
//                    element alone, walks the (uniform) set bits of the band, reads coalesced along b.  No atomics;
//   k_stacked_rowmax sim[i][j] = max over b in mask1[j] of R[i][b]: a wave per pair, coalesced along b, a butterfly of maxima.
// max of finite doubles is exact and order-free: the only rounding is inside c, whose sums have a fixed order.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_min_all(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_max_all(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// One submap's selection by ONE WAVE — what a wave of k_frame_select and of k_session_frame_select_list does once it knows its submap:
// n rows of `src` (indices into the N rows of seg_times), the Nf frames, and `words` mask words at `mask` (words >= ceil(Nf / 64):
// whatever lies beyond the frames is written as zero).  CMP: lane 0 compares every word and the count with what the slot held
// before it stores them -> whether one differs (lane 0's value; false without CMP).
template <bool CMP>
__device__ __forceinline__ bool frame_select_submap(const roman_frame_select_params_t& P, int lane, int n, const int32_t* __restrict__ src, int N,
                                                    const double* __restrict__ seg_times, int Nf, const double* __restrict__ frame_times,
                                                    const double* __restrict__ frame_pos, int words, unsigned long long* __restrict__ mask,
                                                    int32_t* __restrict__ n_sel, double* __restrict__ span)
{
    double lo = INFINITY, hi = -INFINITY;
    for (int r = lane; r < n; r += 64) {
        const int64_t k = src[r];
        if (k < 0 || k >= N) continue;                           // (not what roman_submaps_dev writes: never read out of the table)
        lo = fmin(lo, seg_times[2 * k]); hi = fmax(hi, seg_times[2 * k + 1]);
    }
    lo = wave_min_all(lo); hi = wave_max_all(hi);
    double lx = 0.0, ly = 0.0, lz = 0.0;                         // the last selected candidate (uniform)
    bool have = false, differs = false;
    int total = 0;
    for (int w = 0; w < words; ++w) {
        const int f = 64 * w + lane;
        bool cand = false;
        double px = 0.0, py = 0.0, pz = 0.0;
        if (f < Nf) {
            const double t = frame_times[f];
            cand = lo <= t && t <= hi;
            if (P.thin && cand) { px = frame_pos[3 * (int64_t)f]; py = frame_pos[3 * (int64_t)f + 1]; pz = frame_pos[3 * (int64_t)f + 2]; }
        }
        unsigned long long m = __ballot(cand), sel = m;
        if (P.thin) {
            sel = 0ull;
            while (m) {                                          // (uniform) ascending frame index [REF :236-240]
                const int t = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                const double x = __shfl(px, t), y = __shfl(py, t), z = __shfl(pz, t);
                bool take = !have;
                if (have) {
                    const double dx = x - lx, dy = y - ly, dz = z - lz;
                    take = sqrt((dx * dx + dy * dy) + dz * dz) >= P.thin_dist;
                }
                if (take) { sel |= 1ull << t; lx = x; ly = y; lz = z; have = true; }
            }
        }
        if (lane == 0) {
            if (CMP) differs |= mask[w] != sel;
            mask[w] = sel;
        }
        total += __popcll(sel);
    }
    if (lane == 0) {
        if (CMP) differs |= *n_sel != total;
        *n_sel = total; span[0] = lo; span[1] = hi;
    }
    return differs;
}

__global__ void __launch_bounds__(256) k_frame_select(roman_frame_select_params_t P, int S, int cap, const int32_t* __restrict__ count,
                                                      const int32_t* __restrict__ src, int N, const double* __restrict__ seg_times,
                                                      int Nf, const double* __restrict__ frame_times, const double* __restrict__ frame_pos,
                                                      unsigned long long* __restrict__ mask, int32_t* __restrict__ n_sel, double* __restrict__ span)
{
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;                                          // (wave-uniform)
    const int W = (Nf + 63) >> 6;
    frame_select_submap<false>(P, lane, min(count[s], cap), src + (int64_t)s * cap, N, seg_times, Nf, frame_times, frame_pos, W, mask + (int64_t)s * W,
                               n_sel + s, span + 2 * (int64_t)s);
}

// One robot of a session's frame tensors (roman_session_frame_robot_t as the library stages it): its ranges of the session's tables.
struct SessionFrameRobot {
    int64_t seg0;            // first row of its segment table
    int64_t mask_off;        // word offset of its first mask row
    int32_t n_seg, sub0, n_sub, frame0, n_frames, mask_words;
    int32_t reserved[2];
};
static_assert(sizeof(SessionFrameRobot) == sizeof(roman_session_frame_robot_t), "the staged record is the C ABI's");

// the robot that holds global slot g: the last one whose first slot is <= g (robots without submaps share their first slot with the
// robot behind them, which is the one found).  R >= 1 and g inside the session are the host's to check.
__device__ __forceinline__ int session_frame_robot(const SessionFrameRobot* __restrict__ robots, int R, int g)
{
    int lo = 0, hi = R - 1;
    while (lo < hi) {                                            // (uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (robots[mid].sub0 <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ONE WAVE per LISTED slot, four per workgroup: k_frame_select's body over the robot's ranges of the session's
// tensors, all mask_words of the row written, changed[l] = a word or the count differs from what the slot held.
__global__ void __launch_bounds__(256) k_session_frame_select_list(roman_frame_select_params_t P, int L, int R, const int32_t* __restrict__ list,
                                                                   const SessionFrameRobot* __restrict__ robots, int cap,
                                                                   const int32_t* __restrict__ count, const int32_t* __restrict__ src,
                                                                   const double* __restrict__ seg_times, const double* __restrict__ frame_times,
                                                                   const double* __restrict__ frame_pos, unsigned long long* __restrict__ mask,
                                                                   int32_t* __restrict__ n_sel, double* __restrict__ span, int32_t* __restrict__ changed)
{
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= L) return;                                          // (wave-uniform)
    const int g = list[l];
    const SessionFrameRobot rb = robots[session_frame_robot(robots, R, g)];
    const bool differs = frame_select_submap<true>(P, lane, min(count[g], cap), src + (int64_t)g * cap, rb.n_seg, seg_times + 2 * rb.seg0, rb.n_frames,
                                                   frame_times + rb.frame0, frame_pos ? frame_pos + 3 * (int64_t)rb.frame0 : nullptr, rb.mask_words,
                                                   mask + rb.mask_off + (int64_t)(g - rb.sub0) * rb.mask_words, n_sel + g, span + 2 * (int64_t)g);
    if (lane == 0) changed[l] = differs ? 1 : 0;
}

// column c of the selected rows of one submap, added in ascending frame index
__device__ __forceinline__ double frame_column_sum(int words, int d, int c, const double* __restrict__ frame_desc, const unsigned long long* __restrict__ mask)
{
    double acc = 0.0;
    for (int w = 0; w < words; ++w) {
        unsigned long long bits = mask[w];                       // (uniform)
        while (bits) {
            const int t = __ffsll((long long)bits) - 1;
            bits &= bits - 1ull;
            acc += frame_desc[(int64_t)(64 * w + t) * d + c];
        }
    }
    return acc;
}

// grid (submaps, column groups): mean[s][c] = (sum over the selected frames of submap s, ascending, of column c) / n_sel
__global__ void __launch_bounds__(256) k_frame_mean(int Nf, int d, const double* __restrict__ frame_desc, const unsigned long long* __restrict__ mask,
                                                    const int32_t* __restrict__ n_sel, double* __restrict__ mean)
{
    const int s = blockIdx.x, c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= d) return;
    const int W = (Nf + 63) >> 6;
    mean[(int64_t)s * d + c] = frame_column_sum(W, d, c, frame_desc, mask + (int64_t)s * W) / (double)n_sel[s];   // 0 / 0 = NaN for a submap that selects nothing, as NumPy gives
}

// grid (LISTED slots, column groups), behind k_session_frame_select_list on the same stream: the mean row of every listed slot in
// k_frame_mean's order.  A thread compares its column's old 64 bits with the new ones (NaN by bits) and stores 1 into changed[l]
// only when they differ: every writer stores the same value, no atomic.
__global__ void __launch_bounds__(256) k_session_frame_mean_list(int R, const int32_t* __restrict__ list, const SessionFrameRobot* __restrict__ robots, int d,
                                                                 const double* __restrict__ frame_desc, const unsigned long long* __restrict__ mask,
                                                                 const int32_t* __restrict__ n_sel, double* __restrict__ mean, int32_t* __restrict__ changed)
{
    const int l = blockIdx.x, c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= d) return;
    const int g = list[l];
    const SessionFrameRobot rb = robots[session_frame_robot(robots, R, g)];
    // (a robot without frames selects nothing: its descriptor rows are never read)
    const double v = frame_column_sum((rb.n_frames + 63) >> 6, d, c, frame_desc + (int64_t)rb.frame0 * d,
                                      mask + rb.mask_off + (int64_t)(g - rb.sub0) * rb.mask_words) / (double)n_sel[g];
    double* out = mean + (int64_t)g * d + c;
    if (__double_as_longlong(*out) != __double_as_longlong(v)) changed[l] = 1;
    *out = v;
}

__global__ void __launch_bounds__(256) k_fill_f64(int64_t n, double v, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

constexpr int STACK_TILE = 32;                                   // rows and columns of the frame-cosine matrix a wave of k_stacked_band owns

// One STACK_TILE x STACK_TILE tile (xt, yt) of a band — what a wave of k_stacked_band and of k_session_band does once it knows its
// tile: rows [a0, a0 + H) of desc0 against the Nf1 rows of desc1 -> Cb[H][Nf1].  The contraction order of an element depends on d
// alone, never on the tile, the band or the launch: that is what makes a session's block bit for bit roman_stacked_sim_dev's.
// (stacked_contract(), k_session_stacked_list's, is a copy of the contraction loop below: a change here must be made there too.)
__device__ __forceinline__ void stacked_tile(int d, int a0, int H, int Nf1, const double* desc0, const double* desc1, const double* norm0, const double* norm1,
                                             double* Cb, int xt, int yt)
{
    const int lane = threadIdx.x & 63, lr = lane & 15, kq = lane >> 4;
    const double* fa[2]; const double* fb[2]; bool va[2], vb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ia = STACK_TILE * xt + 16 * h + lr, jb = STACK_TILE * yt + 16 * h + lr;
        va[h] = ia < H; vb[h] = jb < Nf1;
        fa[h] = desc0 + (int64_t)(a0 + (va[h] ? ia : 0)) * d + 4 * kq;      // (an invalid row reads the band's first: in bounds, multiplied as 0)
        fb[h] = desc1 + (int64_t)(vb[h] ? jb : 0) * d + 4 * kq;
    }
    double4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = double4_t{0.0, 0.0, 0.0, 0.0};
    const int nfull = d >> 4;
    for (int c = 0; c < nfull; ++c) {
        d4u_t ra[2], rb[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) { ra[h] = *reinterpret_cast<const d4u_t*>(fa[h] + 16 * c); rb[h] = *reinterpret_cast<const d4u_t*>(fb[h] + 16 * c); }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[x] ? ra[x].v[t] : 0.0, vb[y] ? rb[y].v[t] : 0.0, acc[x][y], 0, 0, 0);
    }
    const int k0 = 16 * nfull;
    if (k0 < d) {                                                // ragged tail of the descriptor (< 16 elements)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool vk = k0 + 4 * kq + t < d;
            double av[2], bv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) { av[h] = (va[h] && vk) ? fa[h][k0 + t] : 0.0; bv[h] = (vb[h] && vk) ? fb[h][k0 + t] : 0.0; }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
        }
    }
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        const int col = STACK_TILE * yt + 16 * y + lr;
        const double nb = col < Nf1 ? norm1[col] : 0.0;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = STACK_TILE * xt + 16 * x + kq + 4 * r;
                if (row < H && col < Nf1) {
                    const double np_ = norm0[a0 + row] * nb;
                    Cb[(int64_t)row * Nf1 + col] = (np_ <= 1e-9) ? 0.0 : acc[x][y][r] / np_;       // [REF roman/map/map.py:159-161]
                }
            }
    }
}

// rows [a0, a0 + H) of map 0 (a0 + H <= Nf0) against the Nf1 frames of map 1 -> Cb[H][Nf1]
__global__ void __launch_bounds__(256) k_stacked_band(int d, int a0, int H, int Nf1, const double* __restrict__ desc0, const double* __restrict__ desc1,
                                                      const double* __restrict__ norm0, const double* __restrict__ norm1, double* __restrict__ Cb)
{
    const int nty = (Nf1 + STACK_TILE - 1) / STACK_TILE, ntx = (H + STACK_TILE - 1) / STACK_TILE;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (int64_t)ntx * nty) return;                         // (wave-uniform)
    stacked_tile(d, a0, H, Nf1, desc0, desc1, norm0, norm1, Cb, (int)(w / nty), (int)(w % nty));
}

// element (i, b) of R against one band — the owner thread's work in k_stacked_colmax and k_session_colmax; `first`: the band opens R
// (nothing is read)
__device__ __forceinline__ void stacked_colmax_one(int i, int b, int W0, int a0, int H, int Nf1, int first, const unsigned long long* mask0, const double* Cb,
                                                   double* R)
{
    double m = first ? -INFINITY : R[(int64_t)i * Nf1 + b];
    for (int w = a0 >> 6; w <= (a0 + H - 1) >> 6; ++w) {
        unsigned long long bits = mask0[(int64_t)i * W0 + w];    // (uniform); clipped to the band's frames
        const int lo = max(a0 - 64 * w, 0), hi = min(a0 + H - 64 * w, 64);
        if (lo > 0) bits &= ~0ull << lo;
        if (hi < 64) bits &= (1ull << hi) - 1ull;
        while (bits) {
            const int t = __ffsll((long long)bits) - 1;
            bits &= bits - 1ull;
            m = fmax(m, Cb[(int64_t)(64 * w + t - a0) * Nf1 + b]);
        }
    }
    R[(int64_t)i * Nf1 + b] = m;
}

// nbx workgroups per submap i
__global__ void __launch_bounds__(256) k_stacked_colmax(int nbx, int W0, int a0, int H, int Nf1, int first, const unsigned long long* __restrict__ mask0,
                                                        const double* __restrict__ Cb, double* __restrict__ R)
{
    const int i = blockIdx.x / nbx, b = (blockIdx.x % nbx) * 256 + threadIdx.x;
    if (b >= Nf1) return;
    stacked_colmax_one(i, b, W0, a0, H, Nf1, first, mask0, Cb, R);
}

// max over b in mask1[j] of R[i][b], the same bits in every lane of the wave — a pair's work in k_stacked_rowmax and k_session_rowmax
__device__ __forceinline__ double stacked_rowmax_one(int i, int j, int W1, int Nf1, const unsigned long long* mask1, const double* R)
{
    const int lane = threadIdx.x & 63;
    double m = -INFINITY;
    for (int w = 0; w < W1; ++w) {
        const unsigned long long bits = mask1[(int64_t)j * W1 + w];      // (uniform)
        const int b = 64 * w + lane;
        if (((bits >> lane) & 1ull) && b < Nf1) m = fmax(m, R[(int64_t)i * Nf1 + b]);
    }
    return wave_max_all(m);
}

__global__ void __launch_bounds__(256) k_stacked_rowmax(int S0, int S1, int W1, int Nf1, const unsigned long long* __restrict__ mask1,
                                                        const double* __restrict__ R, double* __restrict__ sim)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= (int64_t)S0 * S1) return;                           // (wave-uniform)
    const double m = stacked_rowmax_one((int)(p / S1), (int)(p % S1), W1, Nf1, mask1, R);
    if (lane == 0) sim[p] = m;
}

// ---------------------------------------------------------------------------------------------
// The stacked similarity of every block of a session (roman_session_stacked_sim*): roman_stacked_sim_dev over a LIST
// of robot pairs that share ONE frame table.  View r names the frames [frame_lo[r], frame_lo[r] + frame_n[r]) of it and the masks
// uint64[n_r][ceil(frame_n[r] / 64)] at mask + mask_off[r] (bit t: frame frame_lo[r] + t); blocks, sub_off and pair_off are
// k_session_gate's.  The host cuts every live block (submaps and frames on both sides) into ITEMS — (block, a0, h): the rows
// [a0, a0 + h) of the block's frame-cosine matrix — and deals them into ROUNDS of at most ONE item per block, whose bands lie side by
// side in the band workspace.  A round is two launches:
//   k_session_band    a wave per tile of the round: its item by a wave-uniform binary search of the items' tile prefix (as
//                     k_session_gate finds its block), then stacked_tile() — k_stacked_band's wave, instruction for instruction;
//   k_session_colmax  a workgroup per (item, submap i, 256 columns): its item by the workgroup prefix, then stacked_colmax_one().  One
//                     item per block and round: no two threads of a launch own the same element of R, and the rounds are ordered on
//                     the stream — a block's R is opened by its first item (a0 == 0) and updated in place by the later ones.
// Behind the last round:
//   k_session_rowmax  a wave per pair of pair_off[nb]: its block by binary search of pair_off, then stacked_rowmax_one(); -inf for a
//                     block with a view without frames (there is no R to read).
// No atomics, no spin-waits, no cooperative launch; max of doubles is exact and order-free, so how the host cuts the items
// (roman_ctx_set_stacked_band, the other blocks of the list) changes no bit of the result.
// ---------------------------------------------------------------------------------------------
struct SsTab { int nb; const int32_t* sub_off; const int32_t* blocks; const int64_t* pair_off; const int32_t* frame_lo; const int32_t* frame_n; const int64_t* mask_off; };

// rows [a0, a0 + h) of block `block`: its band at band_off of the band workspace (doubles), its block's R at r_off of the R workspace;
// tile_off / wg_off: the tiles / the column-maximum workgroups of the round's items in front of it
struct SsItem { int64_t band_off, tile_off, r_off; int32_t wg_off, block, a0, h; };
static_assert(sizeof(SsItem) == 40, "SsItem travels as five 64-bit words");

// the last k in [0, n) with items[k].tile_off <= x / items[k].wg_off <= x (ascending, items[0] at 0, no item empty)
__device__ __forceinline__ int ss_find_tile(const SsItem* __restrict__ items, int n, int64_t x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (items[mid].tile_off <= x) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ int ss_find_wg(const SsItem* __restrict__ items, int n, int x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (items[mid].wg_off <= x) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(256) k_session_band(int d, SsTab tab, const SsItem* __restrict__ items, int n_items, int64_t tiles,
                                                      const double* __restrict__ desc, const double* __restrict__ norm, double* __restrict__ band)
{
    const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= tiles) return;                                      // (wave-uniform, as everything up to the tile)
    const SsItem it = items[ss_find_tile(items, n_items, w)];
    const int r0 = tab.blocks[4 * it.block], r1 = tab.blocks[4 * it.block + 1];
    const int lo0 = tab.frame_lo[r0], lo1 = tab.frame_lo[r1], Nf1 = tab.frame_n[r1];
    const int nty = (Nf1 + STACK_TILE - 1) / STACK_TILE;
    const int64_t lw = w - it.tile_off;
    stacked_tile(d, it.a0, it.h, Nf1, desc + (int64_t)lo0 * d, desc + (int64_t)lo1 * d, norm + lo0, norm + lo1, band + it.band_off,
                 (int)(lw / nty), (int)(lw % nty));
}

__global__ void __launch_bounds__(256) k_session_colmax(SsTab tab, const SsItem* __restrict__ items, int n_items, const unsigned long long* __restrict__ mask,
                                                        const double* __restrict__ band, double* __restrict__ R)
{
    const SsItem it = items[ss_find_wg(items, n_items, (int)blockIdx.x)];
    const int r0 = tab.blocks[4 * it.block], r1 = tab.blocks[4 * it.block + 1];
    const int Nf0 = tab.frame_n[r0], Nf1 = tab.frame_n[r1];
    const int nbx = (Nf1 + 255) / 256;
    const int lw = (int)blockIdx.x - it.wg_off;
    const int i = lw / nbx, b = (lw % nbx) * 256 + threadIdx.x;
    if (b >= Nf1) return;
    stacked_colmax_one(i, b, (Nf0 + 63) >> 6, it.a0, it.h, Nf1, it.a0 == 0 ? 1 : 0, mask + tab.mask_off[r0], band + it.band_off, R + it.r_off);
}

// r_off[b]: block b's R in the R workspace (read for a live block only)
__global__ void __launch_bounds__(256) k_session_rowmax(SsTab tab, const int64_t* __restrict__ r_off, int64_t total, const unsigned long long* __restrict__ mask,
                                                        const double* __restrict__ R, double* __restrict__ sim)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= total) return;                                      // (wave-uniform)
    const int b = session_find(tab.pair_off, tab.nb, p);
    const int r0 = tab.blocks[4 * b], r1 = tab.blocks[4 * b + 1];
    const int n1 = tab.sub_off[r1 + 1] - tab.sub_off[r1], Nf0 = tab.frame_n[r0], Nf1 = tab.frame_n[r1];
    const int64_t l = p - tab.pair_off[b];
    double m = -INFINITY;                                        // a view without frames: the maximum over nothing
    if (Nf0 > 0 && Nf1 > 0) m = stacked_rowmax_one((int)(l / n1), (int)(l % n1), (Nf1 + 63) >> 6, Nf1, mask + tab.mask_off[r1], R + r_off[b]);
    if (lane == 0) sim[p] = m;
}

// ---------------------------------------------------------------------------------------------
// The stacked similarity of a LIST of pairs of a session (roman_session_stacked_sim_list*): what a growing session
// asks for — only the pairs a new or changed submap touches.  k_grid_norms over the frame table, then
//   k_session_stacked_list  ONE WAVE per listed pair (b, i, j): the entry, its block, the two views and their frame ranges through
//                     scalar loads.  The wave walks the selected frames of mask0[i] in chunks of STACK_TILE (tile rows) and inside
//                     that those of mask1[j] (tile columns); lane (lr, kq) finds the frames of rank 16 h + lr of a chunk by a
//                     wave-uniform walk over the mask words with a running popcount (ss_gather), and the tile is
//                     stacked_contract() over those rows — stacked_tile()'s operations, the row addresses gathered.  The epilogue
//                     divides by the norms as stacked_tile() does and keeps a per-lane maximum; a butterfly, lane 0 stores at the
//                     pair's DENSE position.
// An element's bits depend on d alone (not on its place in a tile), and fmax over one set of doubles does not depend on the order
// (NaN ignored on both sides): the maximum of a pair equals roman_session_stacked_sim_dev's column-then-row maximum bit for bit.
// Nothing is sized by the number of selected frames.  No atomics, no LDS, no scratch.
// ---------------------------------------------------------------------------------------------
// The contraction of one STACK_TILE x STACK_TILE tile over GATHERED rows: lane (lr, kq) holds the rows fa[h] / fb[h] (h = 0, 1: tile
// row / column 16 h + lr, already advanced by 4 kq), va / vb say which of them exist (the others are multiplied as 0).  A SIBLING COPY
// of stacked_tile()'s loop, operation for operation — 2 x 2 blocks of v_mfma_f64_16x16x4, chunks of 16 ascending, step t contracts
// k = 16 c + 4 kq + t, the same 32-byte loads, zero-fill and ragged tail — so the order of an element's sum depends on d alone, not
// on where its row and column sit in the tile nor on where the rows come from.  (One function for both was tried: it cost
// k_stacked_band two VGPRs and k_session_band a wave of occupancy; a change to one loop must be made in the other.)
__device__ __forceinline__ void stacked_contract(int d, int kq, const double* const (&fa)[2], const double* const (&fb)[2], const bool (&va)[2],
                                                 const bool (&vb)[2], double4_t (&acc)[2][2])
{
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = double4_t{0.0, 0.0, 0.0, 0.0};
    const int nfull = d >> 4;
    for (int c = 0; c < nfull; ++c) {
        d4u_t ra[2], rb[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) { ra[h] = *reinterpret_cast<const d4u_t*>(fa[h] + 16 * c); rb[h] = *reinterpret_cast<const d4u_t*>(fb[h] + 16 * c); }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[x] ? ra[x].v[t] : 0.0, vb[y] ? rb[y].v[t] : 0.0, acc[x][y], 0, 0, 0);
    }
    const int k0 = 16 * nfull;
    if (k0 < d) {                                                // ragged tail of the descriptor (< 16 elements)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool vk = k0 + 4 * kq + t < d;
            double av[2], bv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) { av[h] = (va[h] && vk) ? fa[h][k0 + t] : 0.0; bv[h] = (vb[h] && vk) ? fb[h][k0 + t] : 0.0; }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
        }
    }
}

// position of the k-th set bit of x (k < popcount(x)): six halvings, no loop over the bits
__device__ __forceinline__ int ss_nth_bit(unsigned long long x, int k)
{
    int pos = 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int c = __popcll(x & ((1ull << s) - 1ull));
        if (k >= c) { k -= c; x >>= s; pos += s; }
    }
    return pos;
}

// Where a walk over a mask row stands (wave-uniform): word w, and the set bits of the words in front of it
struct SsCursor { int w, cnt; };

// The frames of rank base + 16 h + lr (h = 0, 1) among the set bits of the mask row `m` (W words, bits at Nf and beyond ignored)
// -> idx[h], or -1 where the row selects fewer; returns the selected frames of rank >= base that the chunk holds (0 ..
// STACK_TILE).  `cur` never passes a word that still holds a frame of rank >= base, and is left at the first word the next chunk
// (base + STACK_TILE) needs: chunks are asked for in ascending order.
__device__ __forceinline__ int ss_gather(const unsigned long long* __restrict__ m, int W, int Nf, int base, int lr, SsCursor& cur, int (&idx)[2])
{
    idx[0] = -1; idx[1] = -1;
    int w = cur.w, cnt = cur.cnt;
    while (w < W && cnt < base + STACK_TILE) {                   // (uniform)
        unsigned long long bits = m[w];
        if (64 * w + 64 > Nf) bits &= (1ull << (Nf - 64 * w)) - 1ull;       // (the last word: 0 < Nf - 64 w < 64)
        const int pc = __popcll(bits);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = base + 16 * h + lr - cnt;
            if (k >= 0 && k < pc) idx[h] = 64 * w + ss_nth_bit(bits, k);
        }
        if (cnt + pc > base + STACK_TILE) break;                 // the word holds frames of the next chunk: the cursor stays in front of it
        cnt += pc; ++w;
        cur.w = w; cur.cnt = cnt;
    }
    if (w < W) return STACK_TILE;                                // (left by the break, or by a full chunk: cnt >= base + STACK_TILE)
    return min(max(cnt - base, 0), STACK_TILE);
}

__global__ void __launch_bounds__(256) k_session_stacked_list(int d, SsTab tab, int L, const int32_t* __restrict__ list, const double* __restrict__ desc,
                                                              const double* __restrict__ norm, const unsigned long long* __restrict__ mask,
                                                              double* __restrict__ sim)
{
    const int lane = threadIdx.x & 63, lr = lane & 15, kq = lane >> 4;
    const int64_t l = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (l >= L) return;                                          // (wave-uniform, as everything but the gathered rows)
    const int b = list[3 * l], i = list[3 * l + 1], j = list[3 * l + 2];
    const int r0 = tab.blocks[4 * b], r1 = tab.blocks[4 * b + 1];
    const int n1 = tab.sub_off[r1 + 1] - tab.sub_off[r1];
    const int lo0 = tab.frame_lo[r0], lo1 = tab.frame_lo[r1], Nf0 = tab.frame_n[r0], Nf1 = tab.frame_n[r1];
    const int W0 = (Nf0 + 63) >> 6, W1 = (Nf1 + 63) >> 6;
    const unsigned long long* m0 = mask + tab.mask_off[r0] + (int64_t)i * W0;
    const unsigned long long* m1 = mask + tab.mask_off[r1] + (int64_t)j * W1;
    const double* desc0 = desc + (int64_t)lo0 * d; const double* desc1 = desc + (int64_t)lo1 * d;
    const double* norm0 = norm + lo0; const double* norm1 = norm + lo1;
    double best = -INFINITY;                                     // an empty mask, a view without frames: the maximum over nothing
    if (Nf0 > 0 && Nf1 > 0) {
        SsCursor c0{0, 0};
        for (int bx = 0;; bx += STACK_TILE) {                    // tile rows: the next STACK_TILE selected frames of mask0[i]
            int ia[2];
            const int nx = ss_gather(m0, W0, Nf0, bx, lr, c0, ia);
            if (nx == 0) break;
            const double* fa[2]; bool va[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) { va[h] = ia[h] >= 0; fa[h] = desc0 + (int64_t)(va[h] ? ia[h] : 0) * d + 4 * kq; }   // (an invalid row reads the view's first frame)
            SsCursor c1{0, 0};
            for (int by = 0;; by += STACK_TILE) {                // tile columns: the same over mask1[j]
                int jb[2];
                const int ny = ss_gather(m1, W1, Nf1, by, lr, c1, jb);
                if (ny == 0) break;
                const double* fb[2]; bool vb[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) { vb[h] = jb[h] >= 0; fb[h] = desc1 + (int64_t)(vb[h] ? jb[h] : 0) * d + 4 * kq; }
                double4_t acc[2][2];
                stacked_contract(d, kq, fa, fb, va, vb, acc);
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const double nb = vb[y] ? norm1[jb[y]] : 0.0;
#pragma unroll
                    for (int x = 0; x < 2; ++x)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = __shfl(ia[x], kq + 4 * r);      // tile row 16 x + kq + 4 r: the lane with that lr holds its frame
                            if (row >= 0 && vb[y]) {
                                const double np_ = norm0[row] * nb;
                                best = fmax(best, (np_ <= 1e-9) ? 0.0 : acc[x][y][r] / np_);       // [REF roman/map/map.py:159-161]
                            }
                        }
                }
                if (ny < STACK_TILE) break;
            }
            if (nx < STACK_TILE) break;
        }
    }
    best = wave_max_all(best);
    if (lane == 0) sim[tab.pair_off[b] + (int64_t)i * n1 + j] = best;
}

// elementwise math probe for tests
__global__ void k_debug_math(int kind, const double* __restrict__ a, const double* __restrict__ b,
                             int64_t n, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b ? b[i] : 0.0;
    double r;
    switch (kind) {
    case 0: r = sqrt(x); break;
    case 1: r = exp(x); break;
    case 2: r = cbrt(x); break;
    case 3: r = x / y; break;
    case 4: r = pow(x, y); break;
    case 5: r = fx_exp(x); break;
    case 6: r = fx_cbrt(x); break;
    default: r = fma(x, y, x); break;
    }
    out[i] = r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Segment tables from point clouds: per segment the centre, the three shape ratios of the centred covariance's
// eigenvalues, and extent and volume of the box in its eigenframe — what Segment.minimal_data() computes per segment on the host
// [REF roman/object/segment.py:496-508].  A TEAM of NW waves takes one segment: one wave (k_seg_shapes_wave, four segments per
// workgroup) for a segment of fewer than `block_min` points, the four waves of a workgroup (k_seg_shapes_block) for the others.
// Every sweep reads the cloud as a flat stream of doubles into LDS (coalesced: 24-byte points are not 16-byte aligned), and thread t
// of the team then takes point t of the chunk from there.
//
// Sums run in a FIXED order: thread t of the team adds the points t, t + 64 NW, t + 128 NW, ... of its segment one after the other,
// the 64 lanes of a wave are combined by wave_sum63's tree (6 levels), and the NW waves' sums are added in wave order.  No floating
// point atomics; nothing depends on how waves are scheduled.  The depth of a sum over n terms is ceil(n / (64 NW)) - 1 + 6 + NW - 1.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SEG_BLOCK_MIN = 768;           // ROMAN_SEG_BLOCK_MIN: points from which a segment goes to a workgroup (profiles/segment_shapes/README.md)
constexpr int SEG_ST_EMPTY = 1, SEG_ST_FEW_POINTS = 2, SEG_ST_DEGENERATE = 4;     // ROMAN_SEG_* of include/roman_hip.h

struct SegShapeArgs {
    const double* pts;                       // (P, 3)
    const int64_t* seg_off;                  // [N + 1]
    const int32_t* items;                    // the host-cut list: the segments of the wave kernel, then those of the workgroup kernel
    double* out; int32_t* status;
    int center_ref, stride, col_center, col_pca, col_volume, col_extent;
};

template <int NW> struct SegLds {
    double stage[3 * 64 * NW];               // one chunk of 64 NW points, as it lies in memory
    double red[NW * 6];                      // the waves' partial results of a team reduction
    unsigned long long zkey[NW];
    unsigned int hist[4][256];               // radix select: one histogram per (coordinate, order statistic)
    unsigned long long pre[4];               // ... the key bits found so far
    unsigned int rk[4];                      // ... the rank that is left inside the group of keys that share them
};

// the order-preserving 64-bit key of a double: negative values with every bit flipped, the others with the sign bit set
// (-inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers), and back
__device__ __forceinline__ unsigned long long seg_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double seg_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

template <int NW> __device__ __forceinline__ void seg_sync()
{
    if (NW == 1) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
    else __syncthreads();
}

// One sweep over the n points from row p0 on: f(x, y, z) for every point, in the fixed thread assignment above.  Every thread of
// the team makes every trip of the chunk loop (it holds the team's barriers); ends behind a barrier.
template <int NW, typename F>
__device__ __forceinline__ void seg_sweep(const double* __restrict__ pts, int64_t p0, int64_t n, double* stage, int tid, F f)
{
    constexpr int NT = 64 * NW;
    for (int64_t c0 = 0; c0 < n; c0 += NT) {
        const int m = n - c0 < (int64_t)NT ? (int)(n - c0) : NT;
        const double* src = pts + 3 * (p0 + c0);
#pragma unroll
        for (int k = 0; k < 3; ++k) { const int e = tid + k * NT; if (e < 3 * m) stage[e] = src[e]; }
        seg_sync<NW>();
        if (tid < m) f(stage[3 * tid], stage[3 * tid + 1], stage[3 * tid + 2]);
        seg_sync<NW>();
    }
}

// the team's sum of K values per thread, in the fixed order, on every thread
template <int NW, int K> __device__ __forceinline__ void seg_team_sum(double (&v)[K], double* red, int tid)
{
    static_assert(K <= 6, "SegLds::red holds six values per wave");
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = readlane63(wave_sum63(v[k]));
    if (NW == 1) return;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(tid >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) { double s = red[k]; for (int w = 1; w < NW; ++w) s += red[w * K + k]; v[k] = s; }
    __syncthreads();
}

// the team's minima of lo[3] and maxima of hi[3] (order does not matter to either), on every thread
template <int NW> __device__ __forceinline__ void seg_team_minmax(double (&lo)[3], double (&hi)[3], double* red, int tid)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int off = 32; off > 0; off >>= 1) { lo[k] = fmin(lo[k], __shfl_xor(lo[k], off)); hi[k] = fmax(hi[k], __shfl_xor(hi[k], off)); }
    if (NW == 1) return;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { red[(tid >> 6) * 6 + k] = lo[k]; red[(tid >> 6) * 6 + 3 + k] = hi[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int w = 0; w < NW; ++w) { lo[k] = fmin(lo[k], red[w * 6 + k]); hi[k] = fmax(hi[k], red[w * 6 + 3 + k]); }
    __syncthreads();
}

// Two-sided Jacobi rotation that annihilates A[P][Q] of the symmetric 3 x 3 matrix A; V accumulates the rotations (its columns are
// the eigenvectors).  Indexed at compile time, as jacobi_pair above: A and V stay in registers.
template <int P, int Q> __device__ __forceinline__ void seg_jacobi_rotate(double (&A)[9], double (&V)[9])
{
    constexpr int R = 3 - P - Q;
    const double apq = A[P * 3 + Q];
    if (apq == 0.0) return;
    const double app = A[P * 3 + P], aqq = A[Q * 3 + Q];
    const double a2 = aqq - app, b2 = 2.0 * apq;                // t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = a2 / b2
    const double t = (((a2 >= 0.0) == (b2 >= 0.0)) ? fabs(b2) : -fabs(b2)) / (fabs(a2) + sqrt(a2 * a2 + b2 * b2));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    A[P * 3 + P] = app - t * apq; A[Q * 3 + Q] = aqq + t * apq;
    A[P * 3 + Q] = 0.0; A[Q * 3 + P] = 0.0;
    const double arp = A[R * 3 + P], arq = A[R * 3 + Q];
    A[R * 3 + P] = A[P * 3 + R] = c * arp - s * arq;
    A[R * 3 + Q] = A[Q * 3 + R] = s * arp + c * arq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = V[r * 3 + P], vq = V[r * 3 + Q];
        V[r * 3 + P] = c * vp - s * vq; V[r * 3 + Q] = s * vp + c * vq;
    }
}

// sorts (|e|, column of V) pairs so that e[I] >= e[J]
template <int I, int J> __device__ __forceinline__ void seg_order(double (&e)[3], double (&V)[9])
{
    if (e[I] >= e[J]) return;
    const double t = e[I]; e[I] = e[J]; e[J] = t;
#pragma unroll
    for (int r = 0; r < 3; ++r) { const double v = V[r * 3 + I]; V[r * 3 + I] = V[r * 3 + J]; V[r * 3 + J] = v; }
}

// the bin of the 256-bin histogram h that holds rank r (0-based, r < the histogram's total), and the rank left inside it
__device__ __forceinline__ void seg_find_bin(const unsigned int* h, unsigned int r, int lane, int& bin, unsigned int& rnew)
{
    const unsigned int c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
    const unsigned int s = c0 + c1 + c2 + c3;
    unsigned int incl = s;
    for (int off = 1; off < 64; off <<= 1) { const unsigned int t = (unsigned int)__shfl_up((int)incl, off); if (lane >= off) incl += t; }
    unsigned int e = incl - s;
    const bool hit = r >= e && r < incl;
    int b = 4 * lane;
    if (hit) {
        if (r >= e + c0) { e += c0; ++b; if (r >= e + c1) { e += c1; ++b; if (r >= e + c2) { e += c2; ++b; } } }
    }
    const unsigned long long m = __ballot(hit);
    const int src = m ? (int)__ffsll((long long)m) - 1 : 0;
    bin = __shfl(b, src); rnew = (unsigned int)__shfl((int)(r - e), src);
}

// Radix select over the keys of x and of y, eight passes of eight bits from the top: the order statistics (n - 1) / 2 and n / 2 of
// either coordinate -> their keys in L.pre[0..3] (x low, x high, y low, y high).  Integer LDS histograms only, so the result is
// exact and any n is served with the same 4 KB.
template <int NW>
__device__ __forceinline__ void seg_select_medians(const double* __restrict__ pts, int64_t p0, int64_t n, SegLds<NW>& L, int tid)
{
    constexpr int NT = 64 * NW;
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < 4) { L.pre[tid] = 0ull; L.rk[tid] = (unsigned int)((tid & 1) ? n / 2 : (n - 1) / 2); }
    for (int d = 0; d < 8; ++d) {
        const int shift = 56 - 8 * d;
        const unsigned long long mask = d == 0 ? 0ull : (~0ull << (shift + 8));
        for (int i = tid; i < 4 * 256; i += NT) (&L.hist[0][0])[i] = 0u;
        seg_sync<NW>();
        const unsigned long long pre0 = L.pre[0], pre1 = L.pre[1], pre2 = L.pre[2], pre3 = L.pre[3];
        seg_sweep<NW>(pts, p0, n, L.stage, tid, [&](double x, double y, double) {
            const unsigned long long kx = seg_key(x), ky = seg_key(y);
            const unsigned int bx = (unsigned int)(kx >> shift) & 255u, by = (unsigned int)(ky >> shift) & 255u;
            if ((kx & mask) == pre0) atomicAdd(&L.hist[0][bx], 1u);
            if ((kx & mask) == pre1) atomicAdd(&L.hist[1][bx], 1u);
            if ((ky & mask) == pre2) atomicAdd(&L.hist[2][by], 1u);
            if ((ky & mask) == pre3) atomicAdd(&L.hist[3][by], 1u);
        });
        for (int q = (NW == 1 ? 0 : wave); q < 4; q += (NW == 1 ? 1 : NW)) {
            int bin; unsigned int rnew;
            seg_find_bin(L.hist[q], L.rk[q], lane, bin, rnew);
            if (lane == 0) { L.pre[q] |= (unsigned long long)bin << shift; L.rk[q] = rnew; }
        }
        seg_sync<NW>();
    }
}

template <int NW>
__device__ __forceinline__ void seg_shape_team(const SegShapeArgs& A, int s, SegLds<NW>& L, int tid)
{
    const int64_t p0 = A.seg_off[s], n = A.seg_off[s + 1] - p0;
    double* const row = A.out + (int64_t)s * A.stride;
    if (n <= 0) {                                                // an empty segment: a zero row
        if (tid == 0) {
            for (int k = 0; k < 3; ++k) {
                row[A.col_center + k] = 0.0;
                if (A.col_pca >= 0) row[A.col_pca + k] = 0.0;
                if (A.col_extent >= 0) row[A.col_extent + k] = 0.0;
            }
            if (A.col_volume >= 0) row[A.col_volume] = 0.0;
            A.status[s] = SEG_ST_EMPTY | SEG_ST_FEW_POINTS;
        }
        return;
    }

    // ---- sweep 1: the mean, the smallest z by its key, and whether any point differs from the first ----
    double sum[3] = {0.0, 0.0, 0.0};
    unsigned long long zk = ~0ull;
    const double f0 = A.pts[3 * p0], f1 = A.pts[3 * p0 + 1], f2 = A.pts[3 * p0 + 2];
    int differs = 0;
    seg_sweep<NW>(A.pts, p0, n, L.stage, tid, [&](double x, double y, double z) {
        sum[0] += x; sum[1] += y; sum[2] += z;
        const unsigned long long k = seg_key(z); zk = k < zk ? k : zk;
        differs |= (int)(x != f0) | (int)(y != f1) | (int)(z != f2);
    });
    seg_team_sum<NW, 3>(sum, L.red, tid);
    differs = NW == 1 ? __any(differs) : __syncthreads_or(differs);
    // (n equal points: their mean is that point, exactly — a rounded sum / n may miss it by an ulp, and the covariance of a point
    // cloud without extent is exactly zero, as it is in exact arithmetic)
    const double mean[3] = {differs ? sum[0] / (double)n : f0, differs ? sum[1] / (double)n : f1, differs ? sum[2] / (double)n : f2};

    // ---- sweep 2: the centred covariance (xx xy xz yy yz zz) ----
    double cs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    seg_sweep<NW>(A.pts, p0, n, L.stage, tid, [&](double x, double y, double z) {
        const double dx = x - mean[0], dy = y - mean[1], dz = z - mean[2];
        cs[0] += dx * dx; cs[1] += dx * dy; cs[2] += dx * dz; cs[3] += dy * dy; cs[4] += dy * dz; cs[5] += dz * dz;
    });
    seg_team_sum<NW, 6>(cs, L.red, tid);
#pragma unroll
    for (int k = 0; k < 6; ++k) cs[k] /= (double)n;

    // ---- eigen-decomposition in registers, the same on every thread.  The matrix is first scaled by a power of two so that its
    // largest entry lies in [1, 2): exact, the ratios do not see it, and the squares a rotation forms (a2 * a2 + b2 * b2) can then
    // neither underflow nor overflow, however small or large the cloud (an unscaled covariance below 1e-154 would give 0 / 0 there).
    // Cyclic Jacobi: the off-diagonal part shrinks quadratically from sweep to sweep (1e-3, 1e-6, 1e-12, 1e-24 of the diagonal) and a
    // rotation sets its own entry to an exact 0, so the loop ends either by the test below — 1e-18 is deliberately below the
    // rounding unit: one sweep past working precision, so that the eigenvectors are converged as well — or by three exact zeros;
    // twelve sweeps are a cap for inputs that are not finite, not a count ----
    {
        double mx = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) mx = fmax(mx, fabs(cs[k]));
        if (mx > 0.0 && mx < INFINITY) {
            const int ex = ilogb(mx);
#pragma unroll
            for (int k = 0; k < 6; ++k) cs[k] = scalbn(cs[k], -ex);
        }
    }
    double C[9] = {cs[0], cs[1], cs[2], cs[1], cs[3], cs[4], cs[2], cs[4], cs[5]};
    double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(C[1]) + fabs(C[2]) + fabs(C[5]), dia = fabs(C[0]) + fabs(C[4]) + fabs(C[8]);
        if (off <= 1e-18 * dia) break;
        seg_jacobi_rotate<0, 1>(C, V);
        seg_jacobi_rotate<0, 2>(C, V);
        seg_jacobi_rotate<1, 2>(C, V);
    }
    double e[3] = {fabs(C[0]), fabs(C[4]), fabs(C[8])};         // singular values, as np.linalg.svd gives them [REF roman/object/segment.py:441]
    seg_order<0, 1>(e, V); seg_order<0, 2>(e, V); seg_order<1, 2>(e, V);
    int st = 0;
    if (n <= 4) st |= SEG_ST_FEW_POINTS;
    if (e[0] == 0.0) st |= SEG_ST_DEGENERATE;

    // ---- sweep 3: the box in the eigenframe [REF roman/object/segment.py:244-263] ----
    double ext[3] = {0.0, 0.0, 0.0};
    if (n > 4 && A.col_volume + A.col_extent > -2) {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        seg_sweep<NW>(A.pts, p0, n, L.stage, tid, [&](double x, double y, double z) {
            const double dx = x - mean[0], dy = y - mean[1], dz = z - mean[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double p = (dx * V[k] + dy * V[3 + k]) + dz * V[6 + k];
                lo[k] = fmin(lo[k], p); hi[k] = fmax(hi[k], p);
            }
        });
        seg_team_minmax<NW>(lo, hi, L.red, tid);
#pragma unroll
        for (int k = 0; k < 3; ++k) ext[k] = hi[k] - lo[k];
        if (ext[0] > ext[1]) { const double t = ext[0]; ext[0] = ext[1]; ext[1] = t; }      // ascending: every consumer reads sorted(extent)
        if (ext[1] > ext[2]) { const double t = ext[1]; ext[1] = ext[2]; ext[2] = t; }
        if (ext[0] > ext[1]) { const double t = ext[0]; ext[0] = ext[1]; ext[1] = t; }
    }

    // ---- the centre ----
    double cen[3] = {mean[0], mean[1], mean[2]};
    if (A.center_ref == 1) {                                     // bottom_middle [REF roman/object/segment.py:267-270]
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(zk, off); zk = o < zk ? o : zk; }
        if (NW > 1) {
            if ((tid & 63) == 0) L.zkey[tid >> 6] = zk;
            __syncthreads();
            for (int w = 0; w < NW; ++w) zk = L.zkey[w] < zk ? L.zkey[w] : zk;
        }
        seg_select_medians<NW>(A.pts, p0, n, L, tid);
        const double xa = seg_unkey(L.pre[0]), xb = seg_unkey(L.pre[1]), ya = seg_unkey(L.pre[2]), yb = seg_unkey(L.pre[3]);
        // np.median ends in a mean of the one or two middle values, a sum that starts from +0.0: a median that is a zero is +0.0
        cen[0] = (n & 1) ? 0.0 + xa : ((0.0 + xa) + xb) * 0.5;
        cen[1] = (n & 1) ? 0.0 + ya : ((0.0 + ya) + yb) * 0.5;
        cen[2] = seg_unkey(zk);
    }

    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) row[A.col_center + k] = cen[k];
        if (A.col_pca >= 0) {                                    // [REF roman/object/segment.py:445-472]; 0 / 0 = NaN stays NaN
            row[A.col_pca] = (e[0] - e[1]) / e[0]; row[A.col_pca + 1] = (e[1] - e[2]) / e[0]; row[A.col_pca + 2] = e[2] / e[0];
        }
        if (A.col_volume >= 0) row[A.col_volume] = (ext[0] * ext[1]) * ext[2];
        if (A.col_extent >= 0) { row[A.col_extent] = ext[0]; row[A.col_extent + 1] = ext[1]; row[A.col_extent + 2] = ext[2]; }
        A.status[s] = st;
    }
}

// one wave per listed segment, four to a workgroup; the waves never meet at a workgroup barrier
__global__ void __launch_bounds__(256) k_seg_shapes_wave(SegShapeArgs A, int n_items)
{
    __shared__ SegLds<1> L[4];
    const int wave = (int)threadIdx.x >> 6, it = (int)blockIdx.x * 4 + wave;
    if (it >= n_items) return;
    seg_shape_team<1>(A, A.items[it], L[wave], (int)threadIdx.x & 63);
}

// one workgroup per listed segment, from item `first` of the list on
__global__ void __launch_bounds__(256) k_seg_shapes_block(SegShapeArgs A, int first)
{
    __shared__ SegLds<4> L;
    seg_shape_team<4>(A, A.items[first + (int)blockIdx.x], L, (int)threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Frame data association: voxel IoU / IoM of every (row cloud, column cloud) pair, the cosine of their
// descriptors and the score global_nearest_neighbor puts in front of the Hungarian solve [REF roman/map/global_nearest_neighbor.py:
// 23-36] over VoxelGrid.iou [REF roman/map/voxel_grid.py:32-103].  Integer set operations throughout:
//   1. per cloud the box (float corners as the reference forms them, their TRUNCATED integers) and one 64-bit key per point,
//      three biased 21-bit axes of min_corner_int + grid_index, x the most significant;
//   2. per cloud the keys sorted ascending without duplicates in the cloud's slice of the key workspace, their number = n_vox.
//      A TEAM takes one cloud: one wave (k_assoc_keys_wave, four clouds per workgroup, a bitonic sort in ASSOC_WAVE_CAP keys of
//      LDS), a workgroup sorting in ASSOC_LDS_CAP keys of LDS (k_assoc_keys_block<false>), or a workgroup that sorts LDS-sized
//      chunks and merges them through a global ping-pong of the cloud's own size (k_assoc_keys_block<true>);
//   3. per pair one wave (k_assoc_pairs): the reference's float test on the corners, then the lanes walk the shorter key list,
//      reject keys outside [lo, hi) and binary-search the longer one; ballots sum the hits.
// Counts are integers, so inter, n_vox and geo do not depend on any order; the cosine's sum has a fixed lane order and a fixed
// butterfly.  No atomics anywhere.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int ASSOC_ST_OK = 0, ASSOC_ST_EMPTY = 1, ASSOC_ST_RANGE = 2;          // ROMAN_ASSOC_OK / _EMPTY / _RANGE
constexpr int ASSOC_WAVE_CAP = 512;          // keys of LDS one wave sorts in
constexpr int ASSOC_LDS_CAP = 8192;          // keys of LDS a workgroup sorts in (64 KB)
constexpr int ASSOC_WAVE_MAX = 256;          // ROMAN_ASSOC_WAVE_MAX: a cloud of at most so many points is one wave's (profiles/assoc_scores/README.md)
constexpr int ASSOC_LDS_MAX = ASSOC_LDS_CAP; // ROMAN_ASSOC_LDS_MAX: ... of at most so many is sorted in LDS alone
constexpr long long ASSOC_KEY_BIAS = 1ll << 20;
constexpr unsigned long long ASSOC_KEY_PAD = ~0ull;                            // sorts behind every key (a key has 63 bits)

struct AssocCloud {                          // what stage 3 reads of a cloud
    double minc[3], maxc[3];                 // min_corner, max_corner [REF roman/map/voxel_grid.py:90-91]
    int32_t mci[3], maxci[3];                // min_corner_int, max_corner_int [REF :25-30]
    int32_t n, status;                       // distinct keys; ASSOC_ST_*
};

struct AssocKeyArgs {
    const double* pts;                       // (P, 3)
    const int64_t* off;                      // [NC + 1]
    const int32_t* items;                    // the host-cut list: the clouds of the wave kernel, of the LDS kernel, of the merge kernel
    unsigned long long* keys;                // [P]: cloud c's sorted distinct keys from off[c] on
    unsigned long long* scratch;             // [P]: the merge kernel's other half
    AssocCloud* rec; int32_t* n_vox; int32_t* status;
    double vs; int chunk;                    // voxel size; keys per LDS-sorted chunk of the merge kernel (<= ASSOC_LDS_CAP)
};

template <int NW, int CAP> struct AssocLds {
    double stage[3 * 64 * NW];
    double red[NW * 6];
    int cnt[NW];
    unsigned long long k[CAP];
};

struct AssocBox { double minc[3], maxc[3], origin[3]; long long mci[3], maxci[3]; bool fits; };

// The box of a cloud from its coordinate minima and maxima, in the oracle's operation order (tests/_voxel_oracle.py; the library
// is built with -ffp-contract=off and these are IEEE divisions: the truncation cases depend on the last bit).  fits: every key
// axis + 2^20 is in [0, 2^21).
__device__ __forceinline__ void assoc_box(const double (&mn)[3], const double (&mx)[3], bool finite, double vs, AssocBox& B)
{
#pragma clang fp contract(off)
    B.fits = finite;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        B.minc[k] = floor(mn[k] / vs) * vs;
        B.maxc[k] = ceil(mx[k] / vs) * vs;
        B.origin[k] = mn[k] - vs * 0.5;       // UNPINNED: open3d's documented rule for VoxelGrid.create_from_point_cloud
        const double t = trunc(B.minc[k] / vs), top = t + floor((mx[k] - B.origin[k]) / vs);
        B.fits = B.fits && t >= -(double)ASSOC_KEY_BIAS && top <= (double)(ASSOC_KEY_BIAS - 1);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        B.mci[k] = B.fits ? (long long)(B.minc[k] / vs) : 0ll;                  // astype(int64): toward zero
        B.maxci[k] = B.fits ? (long long)(B.maxc[k] / vs) : 0ll;
    }
}

__device__ __forceinline__ unsigned long long assoc_key(double x, double y, double z, const AssocBox& B, double vs)
{
#pragma clang fp contract(off)
    const long long kx = B.mci[0] + (long long)floor((x - B.origin[0]) / vs) + ASSOC_KEY_BIAS;
    const long long ky = B.mci[1] + (long long)floor((y - B.origin[1]) / vs) + ASSOC_KEY_BIAS;
    const long long kz = B.mci[2] + (long long)floor((z - B.origin[2]) / vs) + ASSOC_KEY_BIAS;
    return ((unsigned long long)kx << 42) | ((unsigned long long)ky << 21) | (unsigned long long)kz;
}

// seg_sweep with the point's index inside the swept range: f(i, x, y, z)
template <int NW, typename F>
__device__ __forceinline__ void assoc_sweep(const double* __restrict__ pts, int64_t p0, int64_t n, double* stage, int tid, F f)
{
    constexpr int NT = 64 * NW;
    for (int64_t c0 = 0; c0 < n; c0 += NT) {
        const int m = n - c0 < (int64_t)NT ? (int)(n - c0) : NT;
        const double* src = pts + 3 * (p0 + c0);
#pragma unroll
        for (int k = 0; k < 3; ++k) { const int e = tid + k * NT; if (e < 3 * m) stage[e] = src[e]; }
        seg_sync<NW>();
        if (tid < m) f(c0 + tid, stage[3 * tid], stage[3 * tid + 1], stage[3 * tid + 2]);
        seg_sync<NW>();
    }
}

// the m keys of k (m a power of two, in LDS) ascending; ends behind a barrier
template <int NW> __device__ __forceinline__ void assoc_bitonic(unsigned long long* k, int m, int tid)
{
    constexpr int NT = 64 * NW;
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (m >> 1); t += NT) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long a = k[i], b = k[j];
                if ((a > b) == ((i & size) == 0)) { k[i] = b; k[j] = a; }
            }
            seg_sync<NW>();
        }
}

// the distinct keys of the ascending src[0..n) -> dst, in order; returns their number on every thread
template <int NW>
__device__ __forceinline__ int assoc_unique(const unsigned long long* src, int64_t n, unsigned long long* __restrict__ dst, int* cnt, int tid)
{
    constexpr int NT = 64 * NW;
    const int lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int64_t c0 = 0; c0 < n; c0 += NT) {
        const int64_t i = c0 + tid;
        unsigned long long v = 0ull;
        bool first = false;
        if (i < n) { v = src[i]; first = i == 0 || src[i - 1] != v; }
        const unsigned long long m = __ballot(first);
        int before = __popcll(m & ((1ull << lane) - 1ull)), total = __popcll(m);
        if (NW > 1) {
            if (lane == 0) cnt[wave] = total;
            __syncthreads();
            total = 0;
            for (int w = 0; w < NW; ++w) { const int c = cnt[w]; if (w < wave) before += c; total += c; }
            __syncthreads();
        }
        if (first) dst[base + before] = v;
        base += total;
    }
    return base;
}

// what the first sweep over a cloud leaves: the box, and the record of a cloud without voxels (returns false for those)
template <int NW>
__device__ __forceinline__ bool assoc_cloud_box(const AssocKeyArgs& A, int c, int64_t p0, int64_t n, double* stage, double* red, int tid, AssocBox& B)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    assoc_sweep<NW>(A.pts, p0, n, stage, tid, [&](int64_t, double x, double y, double z) {
        lo[0] = fmin(lo[0], x); lo[1] = fmin(lo[1], y); lo[2] = fmin(lo[2], z);
        hi[0] = fmax(hi[0], x); hi[1] = fmax(hi[1], y); hi[2] = fmax(hi[2], z);
        bad |= (int)!(fabs(x) < INFINITY) | (int)!(fabs(y) < INFINITY) | (int)!(fabs(z) < INFINITY);
    });
    seg_team_minmax<NW>(lo, hi, red, tid);
    bad = NW == 1 ? __any(bad) : __syncthreads_or(bad);
    if (n > 0) assoc_box(lo, hi, !bad, A.vs, B); else B.fits = false;
    if (B.fits) return true;
    if (tid == 0) {
        AssocCloud R = {};
        R.status = n > 0 ? ASSOC_ST_RANGE : ASSOC_ST_EMPTY;
        A.rec[c] = R; A.status[c] = R.status;
        if (A.n_vox) A.n_vox[c] = 0;
    }
    return false;
}

__device__ __forceinline__ void assoc_cloud_done(const AssocKeyArgs& A, int c, const AssocBox& B, int n_keys)
{
    AssocCloud R;
#pragma unroll
    for (int k = 0; k < 3; ++k) { R.minc[k] = B.minc[k]; R.maxc[k] = B.maxc[k]; R.mci[k] = (int32_t)B.mci[k]; R.maxci[k] = (int32_t)B.maxci[k]; }
    R.n = n_keys; R.status = ASSOC_ST_OK;
    A.rec[c] = R; A.status[c] = ASSOC_ST_OK;
    if (A.n_vox) A.n_vox[c] = n_keys;
}

__device__ __forceinline__ int assoc_pow2(int n) { int m = 2; while (m < n) m <<= 1; return m; }

// the keys of the points [p0, p0 + len) sorted in L.k (len <= CAP; the padding behind them sorts last)
template <int NW, int CAP>
__device__ __forceinline__ void assoc_sort_chunk(const AssocKeyArgs& A, const AssocBox& B, int64_t p0, int len, AssocLds<NW, CAP>& L, int tid)
{
    const int m = assoc_pow2(len);
    for (int i = len + tid; i < m; i += 64 * NW) L.k[i] = ASSOC_KEY_PAD;
    assoc_sweep<NW>(A.pts, p0, len, L.stage, tid, [&](int64_t i, double x, double y, double z) { L.k[i] = assoc_key(x, y, z, B, A.vs); });
    assoc_bitonic<NW>(L.k, m, tid);
}

// a cloud of at most CAP points: box, keys, sort and compaction without leaving LDS
template <int NW, int CAP>
__device__ __forceinline__ void assoc_cloud_lds(const AssocKeyArgs& A, int c, AssocLds<NW, CAP>& L, int tid)
{
    const int64_t p0 = A.off[c], n = A.off[c + 1] - p0;
    AssocBox B;
    if (!assoc_cloud_box<NW>(A, c, p0, n, L.stage, L.red, tid, B)) return;
    assoc_sort_chunk<NW, CAP>(A, B, p0, (int)n, L, tid);
    const int nk = assoc_unique<NW>(L.k, n, A.keys + p0, L.cnt, tid);
    if (tid == 0) assoc_cloud_done(A, c, B, nk);
}

// one wave per listed cloud of at most ASSOC_WAVE_CAP points, four to a workgroup; the waves never meet at a workgroup barrier
__global__ void __launch_bounds__(256) k_assoc_keys_wave(AssocKeyArgs A, int n_items)
{
    __shared__ AssocLds<1, ASSOC_WAVE_CAP> L[4];
    const int wave = (int)threadIdx.x >> 6, it = (int)blockIdx.x * 4 + wave;
    if (it >= n_items) return;
    assoc_cloud_lds<1, ASSOC_WAVE_CAP>(A, A.items[it], L[wave], (int)threadIdx.x & 63);
}

// One workgroup per listed cloud, from item `first` on.  MERGE false: at most ASSOC_LDS_CAP points, sorted in LDS.  MERGE true:
// any number — chunks of A.chunk keys are sorted in LDS and written to one half of the ping-pong (the cloud's slices of A.keys and
// A.scratch), then runs are merged pairwise, every element finding its place by a binary search in the sibling run (stable: lower
// bound for the left run's elements, upper bound for the right's), until one run is left.  The first half is chosen so that the
// last pass ends in A.scratch; the compaction writes A.keys.  Every write stays inside the cloud's own n elements.
template <bool MERGE>
__global__ void __launch_bounds__(256) k_assoc_keys_block(AssocKeyArgs A, int first)
{
    __shared__ AssocLds<4, ASSOC_LDS_CAP> L;
    const int tid = (int)threadIdx.x, c = A.items[first + (int)blockIdx.x];
    if (!MERGE) { assoc_cloud_lds<4, ASSOC_LDS_CAP>(A, c, L, tid); return; }
    const int64_t p0 = A.off[c], n = A.off[c + 1] - p0;
    AssocBox B;
    if (!assoc_cloud_box<4>(A, c, p0, n, L.stage, L.red, tid, B)) return;
    const int64_t chunk = A.chunk;
    int passes = 0;
    for (int64_t w = chunk; w < n; w <<= 1) ++passes;
    unsigned long long* src = (passes & 1) ? A.keys + p0 : A.scratch + p0;
    unsigned long long* dst = (passes & 1) ? A.scratch + p0 : A.keys + p0;
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int len = n - c0 < chunk ? (int)(n - c0) : (int)chunk;
        assoc_sort_chunk<4, ASSOC_LDS_CAP>(A, B, p0 + c0, len, L, tid);
        for (int i = tid; i < len; i += 256) src[c0 + i] = L.k[i];
        __syncthreads();
    }
    for (int64_t w = chunk; w < n; w <<= 1) {
        for (int64_t i = tid; i < n; i += 256) {
            const int64_t base = i / (2 * w) * (2 * w), mid = base + w < n ? base + w : n, end = base + 2 * w < n ? base + 2 * w : n;
            const unsigned long long v = src[i];
            const bool left = i < mid;
            int64_t lo = left ? mid : base, hi = left ? end : mid;              // the sibling run
            const int64_t s0 = lo;
            while (lo < hi) {
                const int64_t m = (lo + hi) >> 1;
                const unsigned long long o = src[m];
                if (left ? o < v : o <= v) lo = m + 1; else hi = m;
            }
            dst[base + (i - (left ? base : mid)) + (lo - s0)] = v;
        }
        __syncthreads();
        unsigned long long* t = src; src = dst; dst = t;
    }
    const int nk = assoc_unique<4>(src, n, A.keys + p0, L.cnt, tid);            // src is A.scratch here
    if (tid == 0) assoc_cloud_done(A, c, B, nk);
}

// the Euclidean norm of every descriptor: one wave per row, lane l adds the squares of columns l, l + 64, ... in order, then a
// fixed butterfly
__device__ __forceinline__ double assoc_butterfly(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__global__ void __launch_bounds__(256) k_assoc_norms(const double* __restrict__ desc, int d, int rows, double* __restrict__ norm)
{
    const int lane = (int)threadIdx.x & 63, r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (r >= rows) return;
    const double* v = desc + (int64_t)r * d;
    double s = 0.0;
    for (int k = lane; k < d; k += 64) s += v[k] * v[k];
    s = assoc_butterfly(s);
    if (lane == 0) norm[r] = sqrt(s);
}

struct AssocPairArgs {
    const AssocCloud* rec; const unsigned long long* keys; const int64_t* off;
    const double* desc; const double* norm; int d;        // d == 0: no descriptors, the cosine is 1.0 [REF roman/map/mapper.py:208-209]
    int N1, N2, col0;                                     // columns are the clouds col0 .. col0 + N2 - 1 (self mode: col0 == 0)
    int iom, semantic;
    double vs3, glo, ghi, slo, shi;                       // voxel_size**3; the two score ranges
    int32_t* inter; double* geo; double* sem; double* score;
};

// one wave per (row, column), four to a workgroup
__global__ void __launch_bounds__(256) k_assoc_pairs(AssocPairArgs A)
{
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (p >= (int64_t)A.N1 * A.N2) return;
    const int i = (int)(p / A.N2), j = A.col0 + (int)(p % A.N2);
    const AssocCloud a = A.rec[i], b = A.rec[j];
    int cnt = 0;
    if (a.n > 0 && b.n > 0) {
        bool open = true;                                  // np.any(min_corner >= max_corner) -> 0.0 [REF roman/map/voxel_grid.py:35-40]
        long long lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            open = open && !(fmax(a.minc[k], b.minc[k]) >= fmin(a.maxc[k], b.maxc[k]));
            lo[k] = (a.mci[k] > b.mci[k] ? a.mci[k] : b.mci[k]) + ASSOC_KEY_BIAS;
            hi[k] = (a.maxci[k] < b.maxci[k] ? a.maxci[k] : b.maxci[k]) + ASSOC_KEY_BIAS;
            open = open && lo[k] < hi[k];
        }
        if (open) {
            const bool a_short = a.n <= b.n;
            const unsigned long long* S = A.keys + A.off[a_short ? i : j];
            const unsigned long long* Lk = A.keys + A.off[a_short ? j : i];
            const int nS = a_short ? a.n : b.n, nL = a_short ? b.n : a.n;
            for (int s0 = 0; s0 < nS; s0 += 64) {
                bool hit = false;
                if (s0 + lane < nS) {
                    const unsigned long long v = S[s0 + lane];
                    const long long x = (long long)(v >> 42), y = (long long)((v >> 21) & 0x1fffffull), z = (long long)(v & 0x1fffffull);
                    if (x >= lo[0] && x < hi[0] && y >= lo[1] && y < hi[1] && z >= lo[2] && z < hi[2]) {
                        int l = 0, h = nL;
                        while (l < h) { const int m = (l + h) >> 1; if (Lk[m] < v) l = m + 1; else h = m; }
                        hit = l < nL && Lk[l] == v;
                    }
                }
                cnt += __popcll(__ballot(hit));
            }
        }
    }
    // volume = num_occupied * vs**3, intersection = count * vs**3, then [REF roman/map/voxel_grid.py:75-83] in its order
    const double va = (double)a.n * A.vs3, vb = (double)b.n * A.vs3, iv = (double)cnt * A.vs3;
    double geo;
    if (A.iom) { const double m = fmin(va, vb); geo = m == 0.0 ? 0.0 : iv / m; }
    else { const double den = va + vb - iv; geo = den == 0.0 ? 0.0 : iv / den; }
    double sem = 1.0;
    if (A.semantic && A.d > 0) {
        const double* u = A.desc + (int64_t)i * A.d;
        const double* w = A.desc + (int64_t)j * A.d;
        double s = 0.0;
        for (int k = lane; k < A.d; k += 64) s += u[k] * w[k];
        sem = assoc_butterfly(s) / (A.norm[i] * A.norm[j]);
    }
    // [REF roman/map/global_nearest_neighbor.py:27-36]: IEEE comparisons, so a NaN similarity is not below its threshold
    double score;
    if (geo < A.glo || (A.semantic && sem < A.slo)) score = 1e9;
    else if (!A.semantic) score = -geo;
    else score = -sqrt(((geo - A.glo) / (A.ghi - A.glo)) * ((sem - A.slo) / (A.shi - A.slo)));
    if (lane == 0) {
        if (A.inter) A.inter[p] = cnt;
        A.geo[p] = geo; A.score[p] = score;
        if (A.semantic && A.sem) A.sem[p] = sem;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Segment update: what Segment._add_points and _cleanup_points do to a segment's cloud with every associated
// observation, every new segment and every merge [REF roman/object/segment.py:133-193] — append, open3d's voxel_down_sample,
// open3d's remove_statistical_outlier(10, std) — for a list of jobs.  A TEAM (one wave or one workgroup of four) takes one job;
// every array of a job lives in the job's SLOT, n(base) + n(add) elements from the host's prefix sum on, in every workspace.
//   front   assemble base + (posed) added points into the slot of `wpts`, minima and maxima on the way; one (voxel key, input
//           index) pair per point, sorted lexicographically — a bitonic network in LDS (k_integ_front_wave, k_integ_front_block<
//           false>) or LDS-sorted chunks merged through a global ping-pong (k_integ_front_block<true>); then one thread per run of
//           equal keys adds the run's points in index order from 0.0 and divides by the count: the down-sampled cloud, ascending key
//   knn     every down-sampled point's ten smallest squared distances to all of them, kept ascending in ten registers by an
//           unrolled compare-exchange chain (no indexing, no scratch); the columns go through LDS as SoA and every lane reads the
//           same one.  Their square roots are added ascending and divided by their number: avg
//   finish  mean, deviation and threshold of avg in ONE order for every class — lane l of a wave adds the elements l, l + 64, ...
//           from 0.0, then the xor butterfly 32, 16, ..., 1 — and a ballot compaction of the kept points into the output slot
// A (key, index) pair is unique, so every sort gives the same sequence, and every sum has one order: all classes give the same
// bits.  No atomics.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int INTEG_NEIGHBORS = 10;          // nb_neighbors of remove_statistical_outlier [REF roman/object/segment.py:183-184]
constexpr int INTEG_LDS_CAP = 4096;          // (key, index) pairs of LDS a team sorts in (48 KB)
constexpr int INTEG_WAVE_MAX = 256;          // ROMAN_INTEGRATE_WAVE_MAX: a job of at most so many points is one wave's
constexpr int INTEG_LDS_MAX = INTEG_LDS_CAP; // ROMAN_INTEGRATE_LDS_MAX: ... of at most so many is sorted in LDS alone
constexpr int INTEG_KEY_TOP = (1 << 21) - 1; // the largest voxel index an axis of the key holds
constexpr int INTEG_TILE = 256;              // query points of one workgroup of k_integ_knn_tile
constexpr int INTEG_COLS_WAVE = 256, INTEG_COLS_BLOCK = 1024;   // column points staged in LDS at a time, per team

struct IntegJob { int32_t base, add, pose; };                   // roman_integrate_job_t

struct IntegArgs {
    const double* pts; const int64_t* off;   // the clouds
    const double* poses;                     // [n_poses][16], row-major 4 x 4
    const IntegJob* jobs;
    const int64_t* slot;                     // [n_jobs + 1]: the exclusive prefix sum of n(base) + n(add), from the host
    const int64_t* items;                    // the host-cut lists: jobs by class; (job << 32 | query tile) for k_integ_knn_tile
    double* wpts;                            // [total][3]: the assembled cloud
    double* ds;                              // [total][3]: the down-sampled cloud in front of the outlier step
    unsigned long long* keys; unsigned long long* keys2; int32_t* idx; int32_t* idx2;     // [total] each: the merge ping-pong
    int32_t* m;                              // [n_jobs]: down-sampled points that wait for knn and finish (0: the job is done)
    double* avg;                             // [total]: out_avg, or workspace
    double* out_points; int32_t* out_count; int32_t* out_status; double* out_thr;
    double vs, std; int outlier; int chunk;  // voxel size; outlier_std and whether it is in use; pairs per LDS-sorted chunk of the merge
};

template <int NW> struct IntegLds {
    double red[NW * 6];
    int cnt[NW];
    unsigned long long k[INTEG_LDS_CAP];
    int32_t ix[INTEG_LDS_CAP];
};

__device__ __forceinline__ bool integ_less(unsigned long long ka, int32_t ia, unsigned long long kb, int32_t ib)
{
    return ka < kb || (ka == kb && ia < ib);
}

// the m pairs (k, ix) (m a power of two, in LDS) ascending; ends behind a barrier
template <int NW> __device__ __forceinline__ void integ_bitonic(unsigned long long* k, int32_t* ix, int m, int tid)
{
    constexpr int NT = 64 * NW;
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (m >> 1); t += NT) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long a = k[i], b = k[j];
                const int32_t ia = ix[i], ib = ix[j];
                if (integ_less(b, ib, a, ia) == ((i & size) == 0)) { k[i] = b; k[j] = a; ix[i] = ib; ix[j] = ia; }
            }
            seg_sync<NW>();
        }
}

// the position of every flagged thread among the flagged ones of the team, and their number (on every thread)
template <int NW> __device__ __forceinline__ int integ_rank(bool flag, int* cnt, int tid, int& total)
{
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long b = __ballot(flag);
    int before = __popcll(b & ((1ull << lane) - 1ull));
    total = __popcll(b);
    if (NW > 1) {
        if (lane == 0) cnt[wave] = total;
        __syncthreads();
        total = 0;
        for (int w = 0; w < NW; ++w) { const int c = cnt[w]; if (w < wave) before += c; total += c; }
        __syncthreads();
    }
    return before;
}

// open3d's voxel_down_sample over the sorted pairs: one thread per run of equal keys adds the run's points one after another, in
// index order, from 0.0 (open3d's AccumulatedPoint) and divides by double(count); runs are written in key order -> their number
template <int NW>
__device__ __forceinline__ int integ_voxels(const unsigned long long* k, const int32_t* ix, int n, const double* __restrict__ w,
                                            double* __restrict__ dst, int* cnt, int tid)
{
    constexpr int NT = 64 * NW;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int i = c0 + tid;
        unsigned long long v = 0ull;
        bool head = false;
        if (i < n) { v = k[i]; head = i == 0 || k[i - 1] != v; }
        int total;
        const int before = integ_rank<NW>(head, cnt, tid, total);
        if (head) {
            double sx = 0.0, sy = 0.0, sz = 0.0;
            int c = 0;
            for (int r = i; r < n && k[r] == v; ++r) { const double* p = w + 3 * (int64_t)ix[r]; sx += p[0]; sy += p[1]; sz += p[2]; ++c; }
            double* o = dst + 3 * (int64_t)(base + before);
            o[0] = sx / (double)c; o[1] = sy / (double)c; o[2] = sz / (double)c;
        }
        base += total;
    }
    return base;
}

// the job's front: assemble, box, keys, sort, voxel sums
template <int NW, bool MERGE>
__device__ __forceinline__ void integ_front(const IntegArgs& A, int j, IntegLds<NW>& L, int tid)
{
#pragma clang fp contract(off)
    constexpr int NT = 64 * NW;
    const IntegJob J = A.jobs[j];
    const int64_t s0 = A.slot[j];
    const int64_t b0 = J.base >= 0 ? A.off[J.base] : 0;
    const int nb = J.base >= 0 ? (int)(A.off[J.base + 1] - b0) : 0;
    const int64_t a0 = A.off[J.add];
    const int na = (int)(A.off[J.add + 1] - a0), n = nb + na;
    if (na == 0) {                           // _add_points' early return [REF roman/object/segment.py:165-166]: the base as it is
        for (int e = tid; e < 3 * nb; e += NT) A.out_points[3 * s0 + e] = A.pts[3 * b0 + e];
        if (tid == 0) { A.m[j] = 0; A.out_count[j] = nb; A.out_status[j] = nb > 0 ? ASSOC_ST_OK : ASSOC_ST_EMPTY; }
        return;
    }
    double T[12];
    if (J.pose >= 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = A.poses[16 * (int64_t)J.pose + e];
    }
    double* w = A.wpts + 3 * s0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int i = tid; i < n; i += NT) {
        const double* p = i < nb ? A.pts + 3 * (b0 + i) : A.pts + 3 * (a0 + (i - nb));
        double x = p[0], y = p[1], z = p[2];
        if (i >= nb && J.pose >= 0) {        // R p + t row by row [REF roman/object/segment.py:142-147]; the reference's BLAS rounding is UNPINNED
            const double wx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
            const double wy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
            const double wz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
            x = wx; y = wy; z = wz;
        }
        w[3 * i] = x; w[3 * i + 1] = y; w[3 * i + 2] = z;
        lo[0] = fmin(lo[0], x); lo[1] = fmin(lo[1], y); lo[2] = fmin(lo[2], z);
        hi[0] = fmax(hi[0], x); hi[1] = fmax(hi[1], y); hi[2] = fmax(hi[2], z);
        bad |= (int)!(fabs(x) < INFINITY) | (int)!(fabs(y) < INFINITY) | (int)!(fabs(z) < INFINITY);
    }
    seg_sync<NW>();
    seg_team_minmax<NW>(lo, hi, L.red, tid);
    bad = NW == 1 ? __any(bad) : __syncthreads_or(bad);
    // UNPINNED: open3d's documented rule for voxel_down_sample — origin = min_bound - voxel_size / 2, index = floor((p - origin) / voxel_size)
    double origin[3];
    bool fits = !bad;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        origin[k] = lo[k] - A.vs * 0.5;
        fits = fits && floor((hi[k] - origin[k]) / A.vs) <= (double)INTEG_KEY_TOP;
    }
    if (!fits) {
        if (tid == 0) { A.m[j] = 0; A.out_count[j] = 0; A.out_status[j] = ASSOC_ST_RANGE; }
        return;
    }
    auto key_of = [&](int i) {
        const unsigned long long kx = (unsigned long long)(long long)floor((w[3 * i] - origin[0]) / A.vs);
        const unsigned long long ky = (unsigned long long)(long long)floor((w[3 * i + 1] - origin[1]) / A.vs);
        const unsigned long long kz = (unsigned long long)(long long)floor((w[3 * i + 2] - origin[2]) / A.vs);
        return (kx << 42) | (ky << 21) | kz;
    };
    double* dst = A.outlier ? A.ds + 3 * s0 : A.out_points + 3 * s0;
    int m;
    if (!MERGE) {                            // n <= INTEG_LDS_CAP
        const int m2 = assoc_pow2(n);
        for (int i = tid; i < m2; i += NT) { const bool in = i < n; L.k[i] = in ? key_of(i) : ASSOC_KEY_PAD; L.ix[i] = in ? i : 0x7fffffff; }
        seg_sync<NW>();
        integ_bitonic<NW>(L.k, L.ix, m2, tid);
        m = integ_voxels<NW>(L.k, L.ix, n, w, dst, L.cnt, tid);
    } else {
        // chunks of A.chunk pairs sorted in LDS, then runs merged pairwise through the ping-pong: every element finds its place by
        // a binary search in the sibling run (the pairs are distinct).  Every access stays inside the slot's n elements.
        unsigned long long* sk = A.keys + s0; unsigned long long* dk = A.keys2 + s0;
        int32_t* si = A.idx + s0; int32_t* di = A.idx2 + s0;
        const int chunk = A.chunk;
        for (int c0 = 0; c0 < n; c0 += chunk) {
            const int len = n - c0 < chunk ? n - c0 : chunk, m2 = assoc_pow2(len);
            for (int i = tid; i < m2; i += NT) { const bool in = i < len; L.k[i] = in ? key_of(c0 + i) : ASSOC_KEY_PAD; L.ix[i] = in ? c0 + i : 0x7fffffff; }
            seg_sync<NW>();
            integ_bitonic<NW>(L.k, L.ix, m2, tid);
            for (int i = tid; i < len; i += NT) { sk[c0 + i] = L.k[i]; si[c0 + i] = L.ix[i]; }
            seg_sync<NW>();
        }
        for (int64_t wd = chunk; wd < n; wd <<= 1) {
            for (int i = tid; i < n; i += NT) {
                const int64_t base = i / (2 * wd) * (2 * wd), mid = base + wd < n ? base + wd : n, end = base + 2 * wd < n ? base + 2 * wd : n;
                const unsigned long long v = sk[i];
                const int32_t vi = si[i];
                const bool left = i < mid;
                int64_t l = left ? mid : base, h = left ? end : mid;            // the sibling run
                const int64_t l0 = l;
                while (l < h) {
                    const int64_t c = (l + h) >> 1;
                    if (integ_less(sk[c], si[c], v, vi)) l = c + 1; else h = c;
                }
                const int64_t at = base + (i - (left ? base : mid)) + (l - l0);
                dk[at] = v; di[at] = vi;
            }
            seg_sync<NW>();
            unsigned long long* tk = sk; sk = dk; dk = tk;
            int32_t* ti = si; si = di; di = ti;
        }
        m = integ_voxels<NW>(sk, si, n, w, dst, L.cnt, tid);
    }
    if (tid == 0) {
        A.out_status[j] = ASSOC_ST_OK;
        if (A.outlier) A.m[j] = m; else { A.m[j] = 0; A.out_count[j] = m; }
    }
}

// one wave per listed job (a workgroup of one wave: the team's LDS is INTEG_LDS_CAP pairs whatever the cut)
__global__ void __launch_bounds__(64) k_integ_front_wave(IntegArgs A)
{
    __shared__ IntegLds<1> L;
    integ_front<1, false>(A, (int)A.items[blockIdx.x], L, (int)threadIdx.x);
}

// one workgroup per listed job, from item `first` on
template <bool MERGE>
__global__ void __launch_bounds__(256) k_integ_front_block(IntegArgs A, int first)
{
    __shared__ IntegLds<4> L;
    integ_front<4, MERGE>(A, (int)A.items[first + (int)blockIdx.x], L, (int)threadIdx.x);
}

// The mean distance of the query points q0 + tid of job j to their min(10, m) nearest of the job's m down-sampled points, the
// point itself included.  best[] ascends; a candidate enters through ten compare-exchanges with compile-time indices.
template <int NW, int COLS>
__device__ __forceinline__ void integ_knn(const IntegArgs& A, int j, int q0, int m, double* cols, int tid)
{
#pragma clang fp contract(off)
    constexpr int NT = 64 * NW;
    const int64_t s0 = A.slot[j];
    const double* __restrict__ P = A.ds + 3 * s0;
    const int q = q0 + tid;
    const bool valid = q < m;
    const double qx = valid ? P[3 * q] : 0.0, qy = valid ? P[3 * q + 1] : 0.0, qz = valid ? P[3 * q + 2] : 0.0;
    double best[INTEG_NEIGHBORS];
#pragma unroll
    for (int r = 0; r < INTEG_NEIGHBORS; ++r) best[r] = INFINITY;
    double* cx = cols; double* cy = cols + COLS; double* cz = cols + 2 * COLS;
    for (int c0 = 0; c0 < m; c0 += COLS) {
        const int len = m - c0 < COLS ? m - c0 : COLS;
        for (int e = tid; e < len; e += NT) { cx[e] = P[3 * (c0 + e)]; cy[e] = P[3 * (c0 + e) + 1]; cz[e] = P[3 * (c0 + e) + 2]; }
        seg_sync<NW>();
        for (int e = 0; e < len; ++e) {
            const double dx = qx - cx[e], dy = qy - cy[e], dz = qz - cz[e];
            double d = (dx * dx + dy * dy) + dz * dz;
            if (d < best[INTEG_NEIGHBORS - 1]) {
#pragma unroll
                for (int r = 0; r < INTEG_NEIGHBORS; ++r) { const double lo = fmin(best[r], d); d = fmax(best[r], d); best[r] = lo; }
            }
        }
        seg_sync<NW>();
    }
    const int k = m < INTEG_NEIGHBORS ? m : INTEG_NEIGHBORS;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < INTEG_NEIGHBORS; ++r) if (r < k) s += sqrt(best[r]);
    if (valid) A.avg[s0 + q] = s / (double)k;
}

// one wave per listed job, four to a workgroup; the waves never meet at a workgroup barrier.  Sized for the default cut, m <=
// INTEG_WAVE_MAX = 256: every batch of 64 queries stages the job's whole column set again, at most four times there.  A cut raised
// through roman_ctx_set_integrate_cuts (measurement and tests only) restages m / 64 times; such jobs belong to k_integ_knn_tile.
__global__ void __launch_bounds__(256) k_integ_knn_wave(IntegArgs A, int n_items)
{
    __shared__ double cols[4][3 * INTEG_COLS_WAVE];
    const int wave = (int)threadIdx.x >> 6, it = (int)blockIdx.x * 4 + wave;
    if (it >= n_items) return;
    const int j = (int)A.items[it], m = A.m[j];
    for (int q0 = 0; q0 < m; q0 += 64) integ_knn<1, INTEG_COLS_WAVE>(A, j, q0, m, cols[wave], (int)threadIdx.x & 63);
}

// one workgroup per listed (job, query tile); the host lists the tiles of n(base) + n(add) points, those past m end at once
__global__ void __launch_bounds__(256) k_integ_knn_tile(IntegArgs A, int first)
{
    __shared__ double cols[3 * INTEG_COLS_BLOCK];
    const int64_t it = A.items[first + (int64_t)blockIdx.x];
    const int j = (int)(it >> 32), q0 = (int)(it & 0xffffffffll) * INTEG_TILE, m = A.m[j];
    if (q0 >= m) return;
    integ_knn<4, INTEG_COLS_BLOCK>(A, j, q0, m, cols, (int)threadIdx.x);
}

// open3d's remove_statistical_outlier behind the distances: mean and deviation over the m values, the threshold, the kept points
template <int NW>
__device__ __forceinline__ void integ_finish(const IntegArgs& A, int j, int* cnt, int tid)
{
#pragma clang fp contract(off)
    constexpr int NT = 64 * NW;
    const int m = A.m[j];
    if (m == 0) return;                      // the front finished the job
    const int64_t s0 = A.slot[j];
    const double* __restrict__ avg = A.avg + s0;
    const int lane = tid & 63;
    // every wave of the team forms the same two sums in the same order: no exchange between them is needed
    double s = 0.0;
    for (int i = lane; i < m; i += 64) { const double a = avg[i]; if (a > 0.0) s += a; }
    const double mean = assoc_butterfly(s) / (double)m;
    double q = 0.0;
    for (int i = lane; i < m; i += 64) { const double a = avg[i]; if (a > 0.0) q += (a - mean) * (a - mean); }
    const double thr = mean + A.std * sqrt(assoc_butterfly(q) / (double)(m - 1));
    const double* __restrict__ P = A.ds + 3 * s0;
    double* __restrict__ O = A.out_points + 3 * s0;
    int base = 0;
    for (int c0 = 0; c0 < m; c0 += NT) {
        const int i = c0 + tid;
        bool keep = false;
        if (i < m) { const double a = avg[i]; keep = a > 0.0 && a < thr; }
        int total;
        const int before = integ_rank<NW>(keep, cnt, tid, total);
        if (keep) { double* o = O + 3 * (int64_t)(base + before); o[0] = P[3 * i]; o[1] = P[3 * i + 1]; o[2] = P[3 * i + 2]; }
        base += total;
    }
    if (tid == 0) { A.out_count[j] = base; if (A.out_thr) A.out_thr[j] = thr; }
}

__global__ void __launch_bounds__(256) k_integ_finish_wave(IntegArgs A, int n_items)
{
    const int it = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (it >= n_items) return;
    integ_finish<1>(A, (int)A.items[it], nullptr, (int)threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) k_integ_finish_block(IntegArgs A, int first)
{
    __shared__ int cnt[4];
    integ_finish<4>(A, (int)A.items[first + (int)blockIdx.x], cnt, (int)threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Segment clustering: what Segment.final_cleanup does to a segment's cloud when the segment goes inactive
// [REF roman/object/segment.py:195-220] — open3d's cluster_dbscan(eps, min_points), keep the largest cluster — for a list of jobs.
// Every array of a job lives in the job's SLOT, n points from the host's prefix sum on, in every workspace.
//   count   every point's number of neighbours (d2 < eps^2, itself included) over SoA columns in LDS that every lane reads at the
//           same address -> the core flags; parent[i] = i
//   union   every (core, core) neighbour pair i > j is united in a union-find over int32 parent[]: the larger root is hooked under
//           the smaller by an integer atomicMin, retried from the value it returns.  parent[i] <= i always and parents only
//           decrease, so the root of a component is its smallest core index whatever the order of the hooks: the partition and the
//           roots do not depend on the schedule
//   border  every non-core point's smallest root among its core neighbours (-1: noise), written where its parent stood
//   finish  rank of every root among the roots (ballot + scan) = the cluster label; labels; sizes by an integer histogram; the
//           largest cluster, the lowest label among equals; a ballot compaction of its points in input order
// A job of at most CLUS_WAVE_MAX points is one wave's (four jobs per workgroup), of at most CLUS_LDS_MAX one workgroup's — both
// hold the cloud, parent, flags and histogram in LDS and run all four steps in one kernel — a larger one runs count, union and
// border over (job, query tile) workgroups through global memory (k_clus_tile<0 / 1 / 2>) and finish in one workgroup.  Every
// loop that follows parents or retries a hook counts down from the index it starts at.  Integer atomics only: all classes and
// any two calls give the same bytes.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int CLUS_WAVE_MAX = 256;           // ROMAN_CLUSTER_WAVE_MAX: a job of at most so many points is one wave's; also the wave's LDS capacity
constexpr int CLUS_LDS_CAP = 1536;           // points a workgroup holds in LDS: 36 B each (three f64 columns, parent, flag, histogram) = 54 KB,
                                             // two workgroups resident in a CU's 160 KB
constexpr int CLUS_LDS_MAX = CLUS_LDS_CAP;   // ROMAN_CLUSTER_LDS_MAX: ... of at most so many is one workgroup's, resident in LDS
constexpr int CLUS_TILE = 256;               // ROMAN_CLUSTER_TILE: query points of one workgroup of k_clus_tile
constexpr int CLUS_COLS = 1024;              // ROMAN_CLUSTER_COLS: column points k_clus_tile stages in LDS at a time

struct ClusArgs {
    const double* pts; const int64_t* off;   // the clouds
    const int32_t* jobs;                     // [n_jobs]: the cloud of every job
    const int64_t* slot;                     // [n_jobs + 1]: the exclusive prefix sum of the jobs' point counts, from the host
    const int64_t* items;                    // the host-cut lists: jobs by class; (job << 32 | query tile) for k_clus_tile
    int32_t* par; int32_t* aux; int32_t* hist;   // [total] each, the tiled class's: parent / border root, core flag / root rank, cluster sizes
    int32_t* lab;                            // [total]: out_labels, or workspace
    double* out_points; int32_t* out_count; int32_t* out_status; int32_t* out_n_clusters; int32_t* out_kept;
    double eps2; int min_points;
};

template <int CAP> struct ClusLds {
    double x[CAP], y[CAP], z[CAP];
    int32_t par[CAP], aux[CAP], hist[CAP];
    unsigned long long red[4];
    int cnt[4];
};

struct ClusCols { double x[CLUS_COLS], y[CLUS_COLS], z[CLUS_COLS]; int32_t tag[CLUS_COLS]; };

// a word other threads (of other workgroups, in the tiled class) may have written with an atomic: read at the device's coherence point
__device__ __forceinline__ int clus_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// j is a neighbour of i iff (dx dx + dy dy) + dz dz < eps^2, strictly and without contraction: symmetric bit for bit
__device__ __forceinline__ bool clus_near(double qx, double qy, double qz, double cx, double cy, double cz, double eps2)
{
#pragma clang fp contract(off)
    const double dx = qx - cx, dy = qy - cy, dz = qz - cz;
    return (dx * dx + dy * dy) + dz * dz < eps2;
}

// the root above x.  parent[i] <= i and a walk only descends: at most x steps, and the countdown holds whatever the memory says
__device__ __forceinline__ int clus_find(const int32_t* par, int x)
{
    for (int g = x; g > 0; --g) {
        const int p = clus_ld(par + x);
        if (p >= x || p < 0) break;
        x = p;
    }
    return x;
}

// Unites the components of a and b: the larger root goes under the smaller.  atomicMin returns what stood there: the root itself
// (hooked, done) or a smaller parent that another thread put there in between — then that parent is united with b, which also
// mends the link the minimum may just have replaced.  The larger of the two roots strictly decreases from one trip to the
// next, so max(a, b) trips suffice.
__device__ __forceinline__ void clus_unite(int32_t* par, int a, int b)
{
    for (int g = a > b ? a : b; g >= 0; --g) {
        a = clus_find(par, a); b = clus_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

// The last step of a job of n > 0 finite points, for a team of NW waves: par[i] is a parent (core points), the smallest root among
// the core neighbours or -1 (the others); aux[i] != 0 marks the core points; hist[0, n) is 0.  par / aux / hist in LDS, or (GLOBAL) in global memory:
// then every barrier stands behind a device-scope fence, so that what a thread stored is what the others load.
template <int NW, bool GLOBAL>
__device__ __forceinline__ void clus_finish(const ClusArgs& A, int j, int n, const double* __restrict__ P, int64_t s0,
                                            int32_t* par, int32_t* aux, int32_t* hist, int* cnt, unsigned long long* red, int tid)
{
    constexpr int NT = 64 * NW;
    int32_t* lab = A.lab + s0;
    // the rank of every root among the roots, ascending index: the label of its cluster.  It replaces the root's flag
    int nc = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int i = c0 + tid;
        const bool root = i < n && aux[i] != 0 && clus_ld(par + i) == i;
        int total;
        const int before = integ_rank<NW>(root, cnt, tid, total);
        if (root) aux[i] = nc + before;
        nc += total;
    }
    if (GLOBAL) __threadfence();
    seg_sync<NW>();
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int i = c0 + tid;
        if (i < n) {
            int r = clus_ld(par + i);
            if (r >= 0) r = clus_find(par, r);
            const int l = r < 0 ? -1 : clus_ld(aux + r);
            lab[i] = l;
            if (l >= 0) atomicAdd(hist + l, 1);
        }
    }
    if (GLOBAL) __threadfence();
    seg_sync<NW>();
    // the largest cluster, the lowest label among equals: the maximum of (size, ~label)
    unsigned long long best = 0ull;
    for (int k = tid; k < nc; k += NT) {
        const unsigned long long key = ((unsigned long long)(unsigned int)clus_ld(hist + k) << 32) | (unsigned long long)(unsigned int)(0x7fffffff - k);
        best = key > best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int hi = (unsigned int)__shfl_xor((int)(best >> 32), off), lo = (unsigned int)__shfl_xor((int)(best & 0xffffffffull), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        best = o > best ? o : best;
    }
    if (NW > 1) {
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
        for (int w = 0; w < NW; ++w) best = red[w] > best ? red[w] : best;
        __syncthreads();
    }
    const int kept = nc > 0 ? 0x7fffffff - (int)(unsigned int)(best & 0xffffffffull) : -1;
    double* __restrict__ O = A.out_points + 3 * s0;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int i = c0 + tid;
        const bool keep = i < n && kept >= 0 && lab[i] == kept;          // lab[i]: this thread's own store
        int total;
        const int before = integ_rank<NW>(keep, cnt, tid, total);
        if (keep) { double* o = O + 3 * (int64_t)(base + before); o[0] = P[3 * i]; o[1] = P[3 * i + 1]; o[2] = P[3 * i + 2]; }
        base += total;
    }
    if (tid == 0) { A.out_count[j] = base; A.out_status[j] = ASSOC_ST_OK; A.out_n_clusters[j] = nc; if (A.out_kept) A.out_kept[j] = kept; }
}

// what a job without a cluster step leaves: no point (EMPTY) or a coordinate that is not finite (RANGE); labels untouched
__device__ __forceinline__ void clus_refuse(const ClusArgs& A, int j, int status)
{
    A.out_count[j] = 0; A.out_status[j] = status; A.out_n_clusters[j] = 0;
    if (A.out_kept) A.out_kept[j] = -1;
}

// a whole job of n <= CAP points by one team, resident in LDS
template <int NW, int CAP>
__device__ __forceinline__ void clus_team(const ClusArgs& A, int j, ClusLds<CAP>& L, int tid)
{
    constexpr int NT = 64 * NW;
    const int c = A.jobs[j];
    const int64_t p0 = A.off[c], s0 = A.slot[j];
    const int n = (int)(A.off[c + 1] - p0);
    const double* __restrict__ P = A.pts + 3 * p0;
    int bad = n > CAP;                       // the host cuts the classes: never
    for (int i = tid; i < n && i < CAP; i += NT) {
        const double x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
        L.x[i] = x; L.y[i] = y; L.z[i] = z; L.par[i] = i; L.hist[i] = 0;
        bad |= (int)!(fabs(x) < INFINITY) | (int)!(fabs(y) < INFINITY) | (int)!(fabs(z) < INFINITY);
    }
    bad = NW == 1 ? __any(bad) : __syncthreads_or(bad);
    seg_sync<NW>();
    if (n == 0 || bad) {
        if (tid == 0) clus_refuse(A, j, n == 0 ? ASSOC_ST_EMPTY : ASSOC_ST_RANGE);
        return;
    }
    // count -> core flags
    for (int q0 = 0; q0 < n; q0 += NT) {
        const int q = q0 + tid < n ? q0 + tid : n - 1;
        const double qx = L.x[q], qy = L.y[q], qz = L.z[q];
        int cnt = 0;
        for (int e = 0; e < n; ++e) cnt += clus_near(qx, qy, qz, L.x[e], L.y[e], L.z[e], A.eps2) ? 1 : 0;
        if (q0 + tid < n) L.aux[q] = cnt >= A.min_points ? 1 : 0;
    }
    seg_sync<NW>();
    // union over the pairs i > j of core points; the columns end at the wave's last query
    for (int q0 = 0; q0 < n; q0 += NT) {
        const int q = q0 + tid < n ? q0 + tid : n - 1;
        const bool core = q0 + tid < n && L.aux[q] != 0;
        const double qx = L.x[q], qy = L.y[q], qz = L.z[q];
        const int last = q0 + (tid | 63), top = last < n ? last : n;
        for (int e = 0; e < top; ++e)
            if (core && e < q && L.aux[e] != 0 && clus_near(qx, qy, qz, L.x[e], L.y[e], L.z[e], A.eps2)) clus_unite(L.par, q, e);
    }
    seg_sync<NW>();
    // parents -> roots (a concurrent walk meets a parent or a root: both lie above it)
    for (int i = tid; i < n; i += NT) if (L.aux[i] != 0) L.par[i] = clus_find(L.par, i);
    seg_sync<NW>();
    // border points: the smallest root among the core neighbours, where the parent stood (no walk reads a non-core point's)
    for (int q0 = 0; q0 < n; q0 += NT) {
        const int q = q0 + tid < n ? q0 + tid : n - 1;
        const bool border = q0 + tid < n && L.aux[q] == 0;
        const double qx = L.x[q], qy = L.y[q], qz = L.z[q];
        int low = 0x7fffffff;
        for (int e = 0; e < n; ++e)
            if (border && L.aux[e] != 0 && clus_near(qx, qy, qz, L.x[e], L.y[e], L.z[e], A.eps2)) { const int r = L.par[e]; low = r < low ? r : low; }
        if (border) L.par[q] = low == 0x7fffffff ? -1 : low;
    }
    seg_sync<NW>();
    clus_finish<NW, false>(A, j, n, P, s0, L.par, L.aux, L.hist, L.cnt, L.red, tid);
}

// one wave per listed job, four to a workgroup; the waves never meet at a workgroup barrier
__global__ void __launch_bounds__(256) k_clus_wave(ClusArgs A, int n_items)
{
    __shared__ ClusLds<CLUS_WAVE_MAX> L[4];
    const int wave = (int)threadIdx.x >> 6, it = (int)blockIdx.x * 4 + wave;
    if (it >= n_items) return;
    clus_team<1, CLUS_WAVE_MAX>(A, (int)A.items[it], L[wave], (int)threadIdx.x & 63);
}

// one workgroup per listed job, from item `first` on
__global__ void __launch_bounds__(256) k_clus_block(ClusArgs A, int first)
{
    __shared__ ClusLds<CLUS_LDS_CAP> L;
    clus_team<4, CLUS_LDS_CAP>(A, (int)A.items[first + (int)blockIdx.x], L, (int)threadIdx.x);
}

// One workgroup per listed (job, query tile) of the tiled class; a tile past the job's n ends at once.  STAGE 0: count, 1: union,
// 2: border.  The columns go through LDS CLUS_COLS at a time, with their core flags (1) or roots (2; -1: not a core point).
template <int STAGE>
__global__ void __launch_bounds__(256) k_clus_tile(ClusArgs A, int first)
{
    __shared__ ClusCols C;
    const int tid = (int)threadIdx.x;
    const int64_t it = A.items[first + (int64_t)blockIdx.x];
    const int j = (int)(it >> 32), q0 = (int)(it & 0xffffffffll) * CLUS_TILE;
    const int c = A.jobs[j];
    const int64_t p0 = A.off[c], s0 = A.slot[j];
    const int n = (int)(A.off[c + 1] - p0);
    if (q0 >= n) return;
    const double* __restrict__ P = A.pts + 3 * p0;
    int32_t* par = A.par + s0; int32_t* aux = A.aux + s0;
    const bool valid = q0 + tid < n;
    const int q = valid ? q0 + tid : n - 1;
    const double qx = P[3 * q], qy = P[3 * q + 1], qz = P[3 * q + 2];
    const bool core = STAGE != 0 && aux[q] != 0;
    const bool active = valid && (STAGE == 0 || (STAGE == 1) == core);
    if (STAGE != 0 && !__syncthreads_or((int)active)) return;
    const int ncol = STAGE == 1 ? (q0 + CLUS_TILE < n ? q0 + CLUS_TILE : n) : n;     // the union visits the pairs i > j alone
    int acc = STAGE == 2 ? 0x7fffffff : 0;
    for (int c0 = 0; c0 < ncol; c0 += CLUS_COLS) {
        const int len = ncol - c0 < CLUS_COLS ? ncol - c0 : CLUS_COLS;
        for (int e = tid; e < len; e += 256) {
            C.x[e] = P[3 * (c0 + e)]; C.y[e] = P[3 * (c0 + e) + 1]; C.z[e] = P[3 * (c0 + e) + 2];
            if (STAGE == 1) C.tag[e] = aux[c0 + e];
            if (STAGE == 2) C.tag[e] = aux[c0 + e] != 0 ? clus_find(par, c0 + e) : -1;
        }
        __syncthreads();
        if (STAGE == 0) {
            for (int e = 0; e < len; ++e) acc += clus_near(qx, qy, qz, C.x[e], C.y[e], C.z[e], A.eps2) ? 1 : 0;
        } else if (STAGE == 1) {
            const int last = q0 + (tid | 63) - c0, top = last < len ? last : len;
            for (int e = 0; e < top; ++e)
                if (active && c0 + e < q && C.tag[e] != 0 && clus_near(qx, qy, qz, C.x[e], C.y[e], C.z[e], A.eps2)) clus_unite(par, q, c0 + e);
        } else {
            for (int e = 0; e < len; ++e)
                if (active && C.tag[e] >= 0 && clus_near(qx, qy, qz, C.x[e], C.y[e], C.z[e], A.eps2)) acc = C.tag[e] < acc ? C.tag[e] : acc;
        }
        __syncthreads();
    }
    if (STAGE == 0 && valid) { aux[q] = acc >= A.min_points ? 1 : 0; par[q] = q; A.hist[s0 + q] = 0; }
    if (STAGE == 2 && active) par[q] = acc == 0x7fffffff ? -1 : acc;     // no walk reads a non-core point's parent
}

// one workgroup per listed job of the tiled class: the finiteness of its coordinates, then clus_finish over the global arrays
__global__ void __launch_bounds__(256) k_clus_finish_block(ClusArgs A, int first)
{
    __shared__ int cnt[4];
    __shared__ unsigned long long red[4];
    const int tid = (int)threadIdx.x, j = (int)A.items[first + (int)blockIdx.x];
    const int c = A.jobs[j];
    const int64_t p0 = A.off[c], s0 = A.slot[j];
    const int n = (int)(A.off[c + 1] - p0);
    const double* __restrict__ P = A.pts + 3 * p0;
    int bad = 0;
    for (int i = tid; i < n; i += 256) bad |= (int)!(fabs(P[3 * i]) < INFINITY) | (int)!(fabs(P[3 * i + 1]) < INFINITY) | (int)!(fabs(P[3 * i + 2]) < INFINITY);
    bad = __syncthreads_or(bad);
    if (n == 0 || bad) {
        if (tid == 0) clus_refuse(A, j, n == 0 ? ASSOC_ST_EMPTY : ASSOC_ST_RANGE);
        return;
    }
    clus_finish<4, true>(A, j, n, P, s0, A.par + s0, A.aux + s0, A.hist + s0, cnt, red, tid);
}

}  // namespace roman
