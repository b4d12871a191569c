// roman_hip.hip — host side of libroman_hip.so: context, HBM workspace, launch sequence and the
// C ABI declared in include/roman_hip.h.  gfx950 only; no CPU fallback.
//
// A batch is a pure ENQUEUE: the launch sequence never waits for the GPU.  The sizes of the sparse
// pools (candidate bit matrices, matrix entries) depend on the data; they are allocated from estimates —
// exact where the invariant has no single scores (every association is live), otherwise from the ratios
// seen in earlier batches with the same parameters (read back lazily, never waited for), otherwise from a
// heuristic — and the device checks every problem against the capacity it was given: a problem that does
// not fit is skipped with ROMAN_ST_WORKSPACE and the recorded need sizes the next attempt.  The entry
// points that are synchronous anyway (host pointers, stepwise API) retry by themselves.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.hip.h"
#include "switches.h"

using namespace roman;

namespace {

thread_local std::string g_last_error;

// grow-only device buffer
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { (void)hipGetLastError(); want = bytes; e = hipMalloc(&p, want); }
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// grow-only pinned staging of one kind of descriptor (a pageable source makes the runtime stage the copy itself, at several times
// the cost).  An upload out of it is a pure enqueue: the only thing ever waited for is the previous upload, which must have left
// the staging before it is rewritten — so stage() synchronises on the event first and upload() records it behind the copy.
template <typename T> struct PinnedStage {
    T* p = nullptr; size_t cap = 0;
    hipEvent_t ev = nullptr; bool pending = false;
    // the staging, free to be written, for at least n elements
    hipError_t stage(size_t n, T** out) {
        hipError_t e;
        if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
        if (pending) { if ((e = hipEventSynchronize(ev)) != hipSuccess) return e; pending = false; }
        if (cap < n) {
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            const size_t want = n + n / 4 + 64;
            if ((e = hipHostMalloc((void**)&p, sizeof(T) * want, hipHostMallocDefault)) != hipSuccess) { p = nullptr; return e; }
            cap = want;
        }
        *out = p; return hipSuccess;
    }
    // its first n elements into `dst`, behind whatever is queued on `stream`
    hipError_t upload(DevBuf& dst, size_t n, hipStream_t stream) {
        hipError_t e = dst.ensure(sizeof(T) * n);
        if (e == hipSuccess) e = hipMemcpyAsync(dst.p, p, sizeof(T) * n, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(ev, stream);
        if (e == hipSuccess) pending = true;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); if (ev) (void)hipEventDestroy(ev); p = nullptr; cap = 0; ev = nullptr; pending = false; }
};

}  // namespace

constexpr int ROMAN_MAX_PIPELINE = 6;        // workspaces (batches in flight) a context can hold (3 serves the headline; calls of thousands of small
                                             // problems — each as long as its slowest problem — pack better at 6)

struct roman_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 256;
    int num_xcc = 8;                           // XCDs the runtime reports for this device / partition (hipDeviceAttributeNumberOfXccs)
    int wide_teams = -1;                       // team mode of the whole-device solver: -1 automatic, 0 never, 1 / 2 / 4 teams per XCD (roman_ctx_set_wide_teams)
    bool teams_launched = false;               // a launch since the last reset ran in team mode (a ROMAN_ST_INTERNAL record may be a team that could not hold its problem)
    size_t lds_max = 65536;
    bool coop_ok = false;                      // hipLaunchCooperativeKernel available (large-problem solver)
    unsigned long long spin_ticks = 400000000ull;  // bounded waits of the whole-device solver: 4 s in ticks of the device's wall clock
    hipEvent_t coopDone = nullptr;             // behind the most recent cooperative launch of this context
    bool coopIssued = false;
    std::string err;

    // Workspace: every device pool of one batch in flight, its stream and its profiling events.  With
    // roman_ctx_set_pipeline(ctx, 2) consecutive batch calls alternate between two of them (each on its own
    // internal stream), so the straggler tail of one batch's kernels overlaps the next batch's build.  Set 0 also
    // serves the stepwise API.
    struct Workspace {
        hipStream_t stream = nullptr;          // set 0 at depth 1: the context's stream; otherwise internal
        hipEvent_t done = nullptr;             // recorded after the last kernel of a batch call
        bool issued = false;
        // pools (see DESIGN.md "Data layout in HBM")
        DevBuf probs, state, totals, queue;
        DevBuf cosPool, cosDense, tabPool, qtabPool, sTmp, chunkCnt;
        DevBuf lp, li, lj, ls, ld, lza, lzb;                       // per live association, live order
        DevBuf plp, pli, plj, pls, pld, plza, plzb;                // the same in position order (stream layout)
        DevBuf rowCnt, rowPos, perm, sliceWidth, sliceBase, items, maskPool, prefPool, listPool, listOff;
        DevBuf vMu, vCu, vMun, vCun, gU, gUn, uOut, nodesOrig, nSel, widePart, wideSlots, wideBar, wideBm, wideY, wideUp, fbList;
        DevBuf cols16, cols32, vals, colsC, valsC;
        long long capMaskWords = 0, capNnz = 0, capList = 0;       // what the sparse pools hold (elements)
        // staging for the host-pointer entry points
        DevBuf hFeats, hAssoc, hU0, oAssoc, oN, oT, oStatus, oStats, hAux1, hAux2, hAux3;
        DevBuf oAll;                           // outputs of a host-output batch call as ONE block (T | stats | assoc | n | status [| records | accepted | count]): one copy brings it back
        DevBuf lcStage;                        // inputs of the loop-closure tail of roman_align_lc_batch (T_ref | FL | FR | enable | iL | iR)
        DevBuf mnoVals, mnoOut;                // roman_mno_batch*: the masked copy of the matrix values; the solver's per-round block (T | stats | assoc | n | status)
        DevBuf mnoHost;                        // roman_mno_batch (host pointers): the three output arrays on the device
        // totals of the most recent batch on this workspace, copied back without waiting
        BatchTotals* pinnedTotals = nullptr;
        PinnedStage<ProbDesc> probStage;       // staging of the problem descriptors (truly asynchronous upload)
        hipEvent_t totEvent = nullptr;
        bool totPending = false;
        double totMaskBound = 0.0, totSumA = 0.0, totMaxA = 0.0;   // the bounds the pending totals relate to
        unsigned totEpoch = 0;                                     // sizing-history epoch (parameter block) the pending totals were measured under
        // per-stage hipEvent pairs on `stream`
        hipEvent_t evA[ROMAN_STAGE_COUNT] = {nullptr, nullptr, nullptr, nullptr};
        hipEvent_t evB[ROMAN_STAGE_COUNT] = {nullptr, nullptr, nullptr, nullptr};
        bool pending[ROMAN_STAGE_COUNT] = {false, false, false, false};
    } ws[ROMAN_MAX_PIPELINE];
    int cur = 0;                               // workspace the current call works on
    int pipeline = 1;                          // batches in flight (1..3)
    int next_ws = 0;
    hipStream_t istream[ROMAN_MAX_PIPELINE] = {};              // internal streams of the workspaces while pipelining
    int latest_ws = -1;                        // workspace of the most recent pipelined batch call
    hipEvent_t evIn = nullptr;                 // inputs ready on the caller's stream
    // roman_align_batch (host pointers): a batch of more than host_chunk problems is issued as calls of host_chunk problems with
    // host_depth of them in flight (roman_ctx_set_host_batching)
    void* hostOut = nullptr; size_t hostOutCap = 0;            // pinned landing block of the host-output entry points' single read-back
    int host_chunk = 2048, host_depth = 3;     // (config 4, 4096 pairs: 2 x 2048 take 37.7 ms, 8 x 512 41 ms — a call pays its launches and its own solver tail)

    // sizing history: largest observed need relative to what the host can bound before the launch
    struct Hist {
        bool valid = false;                    // at least one batch of this block has reported its totals
        bool tagged = false;                   // params / F below are set
        roman_params_t params; int32_t F = 0;  // the ratios belong to this parameter block
        double rMaxL = 0.0;                    // largest live set / largest association list
        double rMask = 0.0;                    // bit-matrix words / sum of nA * ceil(nA / 64)
        double rNnz = 0.0;                     // matrix slots / sum of nA
        double rList = 0.0;                    // candidate-list elements / sum of nA
        bool smallSeen = false;                // a stream-layout problem of at most SMALL_MAXL live associations has occurred
        bool largeSeen = false;                // ... one of more than SMALL_MAXL
        bool generalSeen = false;              // a problem was left to the general kernels (k_small did not finish it)
        bool cosSeen = false;                  // a batch of this block went through k_cos_sel ...
        double cosDenseFrac = 0.0;             // ... and this share of the latest such batch was left to the dense kernel (too many candidates)
        int cosSkipped = 0;                    // batches since that took the dense kernels for it (every 64th tries the screen again)
    } hist;
    long long cosScreenBatches = 0, cosDenseBatches = 0;     // batches with a cosine stage that took k_cos_sel / the dense kernels
    unsigned histEpoch = 1;                    // bumped whenever the history is reset for another parameter block
    long long skippedTotal = 0;                // problems reported ROMAN_ST_WORKSPACE so far (harvested totals)

    // shared-segment removal (roman_shared_ids_dev / roman_align_lc_batch_ids): problem descriptors (through pinned staging, so that the
    // mark step is a pure enqueue), and the host-pointer call's ids | keep lists | kept counts | gather jobs on the device
    DevBuf shareDesc, shareIds, shareKeep, shareKept, shareJobs;
    PinnedStage<ShareDesc> shareStage;

    // the arrays of a host-pointer stage call on the device (HostMirror).  One buffer serves every such call: each ends with a stream
    // synchronise before it returns, so no two of them ever have the block live at the same time.
    DevBuf hostMirror;

    // RANSAC registration (roman_ransac_batch*): problem descriptors through pinned staging (a pure enqueue)
    DevBuf ransacDesc;
    PinnedStage<RansacDesc> ransacStage;

    // submaps from whole maps (roman_submaps*, roman_submaps_fill*, roman_session_submaps*): one record per launched submap — its
    // centre, where its map and its spill slice start — through pinned staging (a pure enqueue), the dense centres of the maps, and
    // the per-submap spill of candidate lists beyond SUBMAP_LDS_CAND
    DevBuf smJobs, smPts, smSpillKey, smSpillIdx;
    PinnedStage<SubmapJob> smStage;
    DevBuf smListOut;      // the list form's select output: src int32[L * cap], count int32[L], status int32[L] of the listed submaps


    // pass 1 of a grid (roman_grid_gate*): the descriptor norms of both sides
    DevBuf ggNorm;

    // pass 1 of a session (roman_session_gate*): the TODO counts of the compaction's workgroups, scanned in place
    DevBuf sgCount;

    // frame descriptors (roman_frame_select* / roman_stacked_sim*): the frame norms of both maps, one row band of the frame-cosine
    // matrix, and the column maxima R
    DevBuf ssNorm, ssBand, ssR;
    int stacked_band = 0;                      // rows per band (roman_ctx_set_stacked_band); 0: automatic
    // ... of a whole session (roman_session_stacked_sim*): the blocks' R offsets and the items of every round, as 64-bit words
    // through pinned staging (a pure enqueue)
    DevBuf ssItems;
    PinnedStage<int64_t> ssStage;
    // the listed slots of a session's resident frame tables (roman_session_frame_select_list*): the robots' records and the list
    // behind them, as 64-bit words through pinned staging (a pure enqueue)
    DevBuf sfTab;
    PinnedStage<int64_t> sfStage;
    // segment shapes from point clouds (roman_segment_shapes*): the host-cut segment list through pinned staging (a pure enqueue)
    DevBuf segItems;
    PinnedStage<int32_t> segStage;
    int seg_block_min = SEG_BLOCK_MIN;         // points from which a segment takes a workgroup (roman_ctx_set_segment_block_min)
    // association scores (roman_assoc_scores*): the key workspace and its merge half (P keys each), one record and one descriptor
    // norm per cloud, and the host-cut cloud list through pinned staging (a pure enqueue)
    DevBuf asKeys, asScratch, asRec, asNorm, asItems;
    PinnedStage<int32_t> asStage;
    int assoc_wave_max = ASSOC_WAVE_MAX, assoc_lds_max = ASSOC_LDS_MAX;   // the two path cuts (roman_ctx_set_assoc_cuts)
    // segment update (roman_segment_integrate*): every workspace holds one slot of n(base) + n(add) elements per job — the assembled
    // and the down-sampled cloud, the (key, index) pairs and their merge half, the mean distances — then one count per job and the
    // host-cut tables (slot offsets, job lists, query tiles) through pinned staging
    DevBuf sgPts, sgDs, sgKeys, sgKeys2, sgIdx, sgIdx2, sgAvg, sgM, sgItems;
    PinnedStage<int64_t> sgStage;
    int integ_wave_max = INTEG_WAVE_MAX, integ_lds_max = INTEG_LDS_MAX;   // the two class cuts (roman_ctx_set_integrate_cuts)
    // segment clustering (roman_segment_cluster*): one slot of n points per job in every workspace — parent, flag and histogram
    // words of the tiled class, the labels when the caller takes none — and the host-cut tables (slot offsets, job lists, query
    // tiles) through pinned staging
    DevBuf clPar, clAux, clHist, clLab, clItems;
    PinnedStage<int64_t> clStage;
    int clus_wave_max = CLUS_WAVE_MAX, clus_lds_max = CLUS_LDS_MAX;       // the two class cuts (roman_ctx_set_cluster_cuts)

    std::vector<std::pair<const void*, int>> ldsAttr;   // dynamic-LDS limits already set (per kernel function)

    bool profile = false;
    double prof_ms[ROMAN_STAGE_COUNT] = {0, 0, 0, 0};
    int64_t prof_n[ROMAN_STAGE_COUNT] = {0, 0, 0, 0};

    // state of the last single-problem call (stepwise API for the clipperpy shim)
    struct Last {
        bool scored = false, solved = false, dense = false, hascz = false;
        int kind = 1;                      // layout of the problem held by workspace 0 (ProbState.kind)
        DevParams D;
        ProbDesc pd;
        int32_t nA = 0, L = 0, nsel = 0;
        int64_t nnzCap = 0;
        std::vector<int32_t> assoc;        // (nA,2) host copy (explicit list) — empty for all-to-all
        std::vector<int32_t> nodes;        // selected nodes (original association indices)
        std::vector<double> u;             // length nA
        roman_stats_t stats;
        int32_t status = 0;
    } last;
};

#define WS (c->ws[c->cur])

// hipFuncAttributeMaxDynamicSharedMemorySize, raised only when a launch needs more than the function already has
static hipError_t dyn_lds(roman_ctx* c, const void* fn, size_t bytes)
{
    for (auto& e : c->ldsAttr) if (e.first == fn) {
        if ((size_t)e.second >= bytes) return hipSuccess;
        e.second = (int)bytes;
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    }
    c->ldsAttr.emplace_back(fn, (int)bytes);
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

namespace {

int fail(roman_ctx* c, int code, const char* fmt, ...)
{
    char buf[640];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    if (c) c->err = buf; else g_last_error = buf;
    return code;
}

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (void)hipGetLastError(); \
    return fail((c), (e_ == hipErrorOutOfMemory) ? ROMAN_E_NOMEM : ROMAN_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } } while (0)

// The stepwise / host-pointer entry points run on workspace 0 and the context's own stream; work that
// pipelined batch calls still have in flight is drained first.
int use_ws0(roman_ctx* c)
{
    if (c->pipeline >= 2)
        for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) if (c->istream[k]) HIPCHK(c, hipStreamSynchronize(c->istream[k]));
    // a depth-1 batch may still be running on the context's (non-blocking) stream: the blocking copies of the stepwise
    // entry points (null stream) are not ordered against it otherwise
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cur = 0; c->ws[0].stream = c->stream;
    return ROMAN_OK;
}

// smallest x with sqrt(x) >= t  (so  sqrt(x) < t  <=>  x < result ; sqrt is monotone and correctly
// rounded on host and device)
double sqrt_threshold(double t)
{
    if (!(t > 0.0)) return 0.0;
    double x = t * t;
    while (std::sqrt(x) >= t) x = std::nextafter(x, 0.0);
    while (std::sqrt(x) < t) x = std::nextafter(x, INFINITY);
    return x;
}

// host twins of col_pos / val_pos (kernels.hip.h)
inline size_t h_col_pos(bool quad, size_t sbase, uint32_t slot, uint32_t e) { return quad ? sbase + (size_t)(e >> 2) * 256 + slot * 4 + (e & 3u) : sbase + (size_t)e * 64 + slot; }
inline size_t h_val_pos(bool quad, size_t sbase, uint32_t slot, uint32_t e) { return quad ? sbase + (size_t)(e >> 1) * 128 + slot * 2 + (e & 1u) : sbase + (size_t)e * 64 + slot; }

int make_dev_params(roman_ctx* c, const roman_params_t* p, int32_t F, DevParams* D)
{
    if (!p) return fail(c, ROMAN_E_INVALID, "params is NULL");
    if (p->point_dim != 2 && p->point_dim != 3) return fail(c, ROMAN_E_INVALID, "point_dim must be 2 or 3 (got %d)", p->point_dim);
    if (p->invariant != ROMAN_INV_EUCLIDEAN && p->invariant != ROMAN_INV_ROMAN && p->invariant != ROMAN_INV_EUCLIDEAN_PRUNED) return fail(c, ROMAN_E_INVALID, "unknown invariant %d", p->invariant);
    if (p->ratio_feature_dim < 0 || p->ratio_feature_dim > ROMAN_MAX_RATIO_FEATURES) return fail(c, ROMAN_E_INVALID, "ratio_feature_dim out of range");
    if (p->cos_feature_dim < 0) return fail(c, ROMAN_E_INVALID, "cos_feature_dim < 0");
    if (p->drift_aware) return fail(c, ROMAN_E_UNSUPPORTED, "drift_aware is not defined by the reference call sites (always False)");
    if (p->invariant == ROMAN_INV_ROMAN && p->gravity_guided && p->point_dim != 3) return fail(c, ROMAN_E_UNSUPPORTED, "gravity_guided requires point_dim == 3");
    if (p->fusion_method < 0 || p->fusion_method > 2) return fail(c, ROMAN_E_INVALID, "unknown fusion_method");
    if (p->gravity_mode < 0 || p->gravity_mode > 2) return fail(c, ROMAN_E_INVALID, "unknown gravity_mode %d", p->gravity_mode);
    if (p->single_mode < 0 || p->single_mode > 3) return fail(c, ROMAN_E_INVALID, "unknown single_mode %d", p->single_mode);
    if (p->reserved != 0) return fail(c, ROMAN_E_INVALID, "roman_params_t.reserved must be 0");
    if (!(p->sigma > 0.0)) return fail(c, ROMAN_E_INVALID, "sigma must be > 0");
    const int need = (p->invariant != ROMAN_INV_EUCLIDEAN) ? p->point_dim + p->ratio_feature_dim + p->cos_feature_dim : p->point_dim;
    if (F < need) return fail(c, ROMAN_E_INVALID, "F=%d smaller than the %d features the invariant reads", F, need);
    memset(D, 0, sizeof(*D));
    D->p = *p;
    if (p->invariant == ROMAN_INV_EUCLIDEAN) { D->p.ratio_feature_dim = 0; D->p.cos_feature_dim = 0; D->p.gravity_guided = 0; D->p.gravity_mode = 0; D->p.single_mode = 0; }
    D->sig2 = p->sigma * p->sigma;
    D->sin_unc = std::sin(p->gravity_unc_ang_rad);
    D->x_eps = sqrt_threshold(p->epsilon);
    D->x_mindist = sqrt_threshold(p->mindist);
    if (p->invariant == ROMAN_INV_EUCLIDEAN_PRUNED) { D->p.gravity_guided = 0; D->p.gravity_mode = 0; D->p.single_mode = ROMAN_SINGLE_DIAG; }   // the pair score alone in M
    D->single = (p->invariant != ROMAN_INV_EUCLIDEAN) && (p->ratio_feature_dim > 0 || p->cos_feature_dim > 0);
    D->pruned = (p->invariant == ROMAN_INV_EUCLIDEAN_PRUNED && D->single) ? 1 : 0;
    D->gravity = (p->invariant == ROMAN_INV_ROMAN) && p->gravity_guided;
    D->gmode = D->gravity ? 1 + p->gravity_mode : 0;
    D->diag_one = D->single && (D->p.single_mode == ROMAN_SINGLE_OFFDIAG || D->pruned);
    D->keep_all = D->single && D->p.single_mode == ROMAN_SINGLE_DIAG_KEEP;
    D->F = F;
    D->stream_maxL = STREAM_MAXL;
    // k_count's prefilter: bins of epsilon / 32 (15 bits: 1023 epsilon of range, 614 m at the reference's 0.6 m; everything beyond shares the
    // last bin) — a gate-passing pair's entries are at most 32 + 1 bins apart (rounding); one bin of margin: pairs up to 1.09 epsilon apart
    // reach the exact gate (bins of epsilon / 8, the first version: 1.375 epsilon, a quarter more candidates)
    D->pre_invw = (p->epsilon > 0.0 && std::isfinite(p->epsilon)) ? 32.0 / p->epsilon : 0.0;
    D->pre_K = 34;
    D->allow_fallback = 1;
    return ROMAN_OK;
}

void prof_flush(roman_ctx* c, int k, int s)
{
    roman_ctx::Workspace& W = c->ws[k];
    if (!W.pending[s]) return;
    float ms = 0.f;
    if (hipEventSynchronize(W.evB[s]) == hipSuccess && hipEventElapsedTime(&ms, W.evA[s], W.evB[s]) == hipSuccess) {
        c->prof_ms[s] += (double)ms; c->prof_n[s] += 1;
    }
    W.pending[s] = false;
}
struct StageTimer {
    roman_ctx* c; int s;
    StageTimer(roman_ctx* c_, int s_) : c(c_), s(s_) { if (c->profile) { prof_flush(c, c->cur, s); (void)hipEventRecord(WS.evA[s], WS.stream); } }
    void stop() { if (c->profile) { (void)hipEventRecord(WS.evB[s], WS.stream); WS.pending[s] = true; } }
};

// ROMAN_DEBUG=1: synchronise after every launch and say which one it was (locating a kernel that does not return)
int dbg_stage(roman_ctx* c, const char* what)
{
    if (!switches_once().debug) return ROMAN_OK;
    const hipError_t e = hipStreamSynchronize(WS.stream);
    fprintf(stderr, "[roman] %-14s %s\n", what, e == hipSuccess ? "ok" : hipGetErrorString(e));
    fflush(stderr);
    return e == hipSuccess ? ROMAN_OK : fail(c, ROMAN_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
}
#define DBG(c, what) do { int rc_ = dbg_stage((c), (what)); if (rc_) return rc_; } while (0)

struct BatchIn {
    int32_t B; const double* feats; const int64_t* off1; const int32_t* n1; const int64_t* off2; const int32_t* n2;
    int32_t F; const int32_t* assoc; const int64_t* assoc_off;
};

// ---- sizing -----------------------------------------------------------------------------------------------------
// What the host can bound before the launch, and the estimates derived from it.
struct Sizing {
    double sumA = 0, maxA = 0, maskBound = 0;      // sum / max of the association list lengths, sum of nA * ceil(nA/64)
    int expectMaxL = 0;                            // estimate of the largest live set
    long long capMaskWords = 0, capNnz = 0, capList = 0;        // capacities to allocate (elements)
};

// Fold the totals a finished batch left in pinned memory into the history (never waits: only completed copies count).
void harvest_totals(roman_ctx* c, bool wait)
{
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) {
        roman_ctx::Workspace& W = c->ws[k];
        if (!W.totPending || !W.totEvent) continue;
        if (wait) { if (hipEventSynchronize(W.totEvent) != hipSuccess) { (void)hipGetLastError(); continue; } }
        else if (hipEventQuery(W.totEvent) != hipSuccess) { (void)hipGetLastError(); continue; }
        W.totPending = false;
        const BatchTotals& t = *W.pinnedTotals;
        c->skippedTotal += t.overflow;
        if (W.totEpoch != c->histEpoch) continue;               // measured under another parameter block: not this history's ratios
        roman_ctx::Hist& H = c->hist;
        if (W.totMaxA > 0) H.rMaxL = std::max(H.rMaxL, (double)t.maxL / W.totMaxA);
        if (W.totMaskBound > 0) H.rMask = std::max(H.rMask, (double)t.needMaskWords / W.totMaskBound);
        if (W.totSumA > 0) H.rNnz = std::max(H.rNnz, (double)t.needNnz / W.totSumA);
        if (W.totSumA > 0) H.rList = std::max(H.rList, (double)t.listTop / W.totSumA);
        if (t.minStreamL <= SMALL_MAXL) H.smallSeen = true;
        if (t.maxStreamL > SMALL_MAXL) H.largeSeen = true;
        if (t.nGeneral > 0) H.generalSeen = true;
        if (t.cosScreened > 0) { H.cosSeen = true; H.cosDenseFrac = (double)t.cosDense / t.cosScreened; }
        H.valid = true;
    }
}

void estimate_sizes(roman_ctx* c, const Switches& sw, const DevParams& D, const roman_params_t* params, int32_t F, const std::vector<ProbDesc>& hd, Sizing* S)
{
    roman_ctx::Hist& H = c->hist;
    if (!H.tagged || H.F != F || memcmp(&H.params, params, sizeof(roman_params_t)) != 0) {   // other parameters: other ratios
        H = roman_ctx::Hist{}; H.params = *params; H.F = F; H.tagged = true;
        ++c->histEpoch;                                         // totals still in flight belong to the old block: harvest_totals drops them
    }
    harvest_totals(c, false);
    const bool prunes = D.single && !D.keep_all && !D.plain_all;   // single scores can remove associations: L <= A, else L == A
    double heurMask = 0, heurNnz = 0; int heurMaxL = 0;
    for (const ProbDesc& d : hd) {
        const double nA = d.nA;
        S->sumA += nA; S->maxA = std::max(S->maxA, nA); S->maskBound += nA * std::ceil(nA / 64.0);
        // first-call heuristic: without single scores every association is live; with them a fraction is
        const double capL = prunes ? std::min(nA, std::max(4096.0, nA / 8.0)) : nA;
        heurMaxL = std::max(heurMaxL, (int)capL);
        heurMask += capL * std::ceil(capL / 64.0);
        heurNnz += capL * std::min(capL, 96.0);
    }
    if (H.valid) {
        S->expectMaxL = prunes ? (int)std::min(S->maxA, std::ceil(H.rMaxL * S->maxA * 1.15) + 64.0) : (int)S->maxA;
        S->capMaskWords = (long long)(prunes ? H.rMask * S->maskBound * 1.3 + 4096.0 : S->maskBound);
        S->capNnz = (long long)(H.rNnz * S->sumA * 1.3 + 65536.0);
        S->capList = (long long)(H.rList * S->sumA * 1.3 + 65536.0);
    } else {
        S->expectMaxL = heurMaxL; S->capMaskWords = (long long)heurMask; S->capNnz = (long long)heurNnz + 65536;
        S->capList = (long long)(2.5 * heurNnz) + 65536;
    }
    S->capMaskWords = std::max<long long>(S->capMaskWords, 64);
    // tests: force the first attempt of a batch to overflow (exercises the skip / retry path)
    if (sw.test_capnnz_set && !H.valid) S->capNnz = sw.test_capnnz;
    if (sw.test_caplist_set && !H.valid) S->capList = sw.test_caplist;   // ... or its list pool too small (k_lists' overflow: kind 2)
}

int may_fallback(const DevParams& D, const std::vector<ProbDesc>& hd);

struct BatchOut { int32_t kmax; int32_t* assoc_out; int32_t* n_assoc_out; double* T_out; int32_t* status_out; roman_stats_t* stats_out; };

// device pointers of a batch's outputs + the row pools the solvers' shared tail writes (sized by the association total)
int make_solve_out(roman_ctx* c, int B, int64_t sumA, const BatchOut& out, SolveOut* O)
{
    const size_t R1 = (size_t)std::max<int64_t>(sumA, 1);
    HIPCHK(c, WS.uOut.ensure(sizeof(double) * R1)); HIPCHK(c, WS.nodesOrig.ensure(sizeof(int32_t) * R1));
    HIPCHK(c, WS.nSel.ensure(sizeof(int32_t) * (size_t)B));
    O->assoc_out = out.assoc_out; O->n_assoc_out = out.n_assoc_out; O->T_out = out.T_out; O->status_out = out.status_out; O->stats_out = out.stats_out; O->kmax = out.kmax;
    O->nodesOrig = WS.nodesOrig.as<int32_t>(); O->nSel = WS.nSel.as<int32_t>(); O->uOut = WS.uOut.as<double>();
    O->dbg = nullptr;
    return ROMAN_OK;
}

// The cosines of a batch that are only used behind the gate cos > cosine_min: k_cos_sel (bf16 screen of all pairs, exact f64 for the
// candidates), then k_cos_deal for the problems it flagged (more candidates than its list holds).  `approx`: no candidates at all —
// the screen's own matrix (tests).
static hipError_t launch_cos_flagged(roman_ctx* c, hipStream_t stream, const DevParams& D, int B, int maxN1, int maxN2, const ProbDesc* dP, const double* feats,
                                     double* cosPool, const int32_t* dense);
static hipError_t launch_cos_sel(roman_ctx* c, hipStream_t stream, const DevParams& D, int B, int maxN1, int maxN2, const ProbDesc* dP, const double* feats, double* cosPool,
                                 int32_t* dense, bool approx)
{
    hipError_t e = dyn_lds(c, reinterpret_cast<const void*>(k_cos_sel), (size_t)CSEL_LDS);
    if (e != hipSuccess) return e;
    const double thr = approx ? INFINITY : D.p.cosine_min - 0x1p-6;
    hipLaunchKernelGGL(k_cos_sel, dim3((unsigned)B), dim3(1024), (size_t)CSEL_LDS, stream, D, B, dP, feats, cosPool, dense, thr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_cos_flagged(c, stream, D, B, maxN1, maxN2, dP, feats, cosPool, dense);
}
// The cosine stage AND the single scores / live pools of a batch of all-to-all problems (k_cos_live), then, for the problems it flagged,
// k_cos_deal; the launcher runs k_live behind it for those only.
static hipError_t launch_cos_live(roman_ctx* c, hipStream_t stream, const DevParams& D, int B, int maxN1, int maxN2, const ProbDesc* dP, const double* feats, double* cosPool,
                                  int32_t* dense, ProbState* st, const LivePools& LP)
{
    hipError_t e = dyn_lds(c, reinterpret_cast<const void*>(k_cos_live), (size_t)CSEL_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cos_live, dim3((unsigned)B), dim3(1024), (size_t)CSEL_LDS, stream, D, B, dP, feats, dense, D.p.cosine_min - 0x1p-6,
                       st, LP.lp, LP.li, LP.lj, LP.ls, LP.ld, LP.lza, LP.lzb);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_cos_flagged(c, stream, D, B, maxN1, maxN2, dP, feats, cosPool, dense);
}
// k_cos_deal behind k_cos_sel / k_cos_live for the problems they flagged (more candidates than their list holds, maps beyond the block budget)
static hipError_t launch_cos_flagged(roman_ctx* c, hipStream_t stream, const DevParams& D, int B, int maxN1, int maxN2, const ProbDesc* dP, const double* feats,
                                     double* cosPool, const int32_t* dense)
{
    hipError_t e;
    constexpr int TD = 5;
    using CD = CosDeal<TD>;
    const int Gd = CD::tiles(maxN1) * CD::tiles(maxN2);
    e = dyn_lds(c, reinterpret_cast<const void*>(k_cos_deal<TD, 0>), (size_t)CD::LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_cos_deal<TD, 0>), dim3((unsigned)(B >= 8 ? Gd * ((B + 7) / 8) * 8 : Gd * B)), dim3(256), (size_t)CD::LDS, stream, D, B, Gd, dP, feats, cosPool, (const int32_t*)dense);
    return hipGetLastError();
}
// When: the score is the gated one (single scores on, not the pruned prefilter's raw products, cosine_max > cosine_min), maps of at most
// CSEL_MAXN objects, and a batch that gives most compute units a problem.  sw.cos_sel: never / whenever the results allow it (tests).
static bool cos_sel_applies(const roman_ctx* c, const Switches& sw, const DevParams& D, int B, int maxN1, int maxN2, int64_t poolRows)
{
    if (!D.single || D.pruned || !(D.p.cosine_max > D.p.cosine_min) || !std::isfinite(D.p.cosine_min) || !std::isfinite(D.p.cosine_max)) return false;
    if (maxN1 > CSEL_MAXN || maxN2 > CSEL_MAXN || maxN1 <= 0 || maxN2 <= 0) return false;
    if (poolRows * (int64_t)D.F * 8 >= (1LL << 32)) return false;         // (the exact pass addresses a row by a 32-bit byte offset into the pool)
    if (sw.cos_sel != CHOICE_LIB) return sw.cos_sel == 1;
    // by itself: a batch that gives at least half the compute units a problem (one workgroup per problem; smaller batches keep the dense
    // kernels' many workgroups per problem), descriptors long enough for the two sweeps to pay, and no history of this parameter block
    // that says the screen rules out too little (a quarter of the latest screened batch left to the dense kernel: the dense kernel
    // directly, the screen again every 64th batch)
    if (2 * B < c->num_cu || D.p.cos_feature_dim < 64 || std::max(maxN1, maxN2) < 64) return false;
    roman_ctx::Hist& H = const_cast<roman_ctx*>(c)->hist;
    if (H.cosSeen && H.cosDenseFrac > 0.25) {
        if (++H.cosSkipped < 64) return false;
        H.cosSkipped = 0;
    }
    return true;
}

// ---- the launch sequence of one batch (score + solve), on workspace c->cur and its stream; never waits -------------

// Cosine matrices of B problems: k_cos_tile (64x64 tile per workgroup, operands through LDS) by default, k_cos_deal (80x80 tiles, blocks
// dealt evenly to the waves) for batches of mid-size maps, k_cos_wave (one wave per problem) or k_cos_block (one wave per block) for
// maps of at most 48 objects, k_cos_block again for a few problems of larger maps.
static hipError_t launch_cos(roman_ctx* c, const Switches& sw, hipStream_t stream, const DevParams& D, int B, int maxN1, int maxN2, const ProbDesc* dP, const double* feats, double* cosPool)
{
    {   // a batch with at least two workgroups per compute unit of 5 x 5-block tiles: k_cos_deal (blocks dealt evenly to the waves).
        // sw.cos_deal: never / always (A/B, tests)
        constexpr int TD = 5;
        using CD = CosDeal<TD>;
        const int Gd = CD::tiles(maxN1) * CD::tiles(maxN2);
        const bool deal = sw.cos_deal != CHOICE_LIB ? sw.cos_deal == 1 : ((maxN1 > 16 * COSW_NB || maxN2 > 16 * COSW_NB) && (int64_t)Gd * B >= 2 * (int64_t)c->num_cu);
        if (deal) {
            const hipError_t e = dyn_lds(c, reinterpret_cast<const void*>(k_cos_deal<TD, 0>), (size_t)CD::LDS);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((k_cos_deal<TD, 0>), dim3((unsigned)(B >= 8 ? Gd * ((B + 7) / 8) * 8 : Gd * B)), dim3(256), (size_t)CD::LDS, stream, D, B, Gd, dP, feats, cosPool, (const int32_t*)nullptr);
            return hipGetLastError();
        }
    }
    if (maxN1 <= 16 * COSW_NB && maxN2 <= 16 * COSW_NB) {
        // the reference's demo scale: one wave per problem, no LDS, no barrier (k_cos_wave); up to two problems per compute unit (a
        // serial caller's one pair per call, a small batch): one wave per 16 x 16 block (k_cos_block: 31 against 80 us for one pair,
        // 75 against 127 for 256, 114 against 135 for 512, 196 against 152 for 1024 — tools/gpu_cos_block_sweep.py).
        // sw.cos_block: never / always (A/B, tests)
        const bool perBlock = sw.cos_block != CHOICE_LIB ? sw.cos_block == 1 : B <= 2 * c->num_cu;
        const int nbx = (maxN1 + 15) / 16, nby = (maxN2 + 15) / 16;
        if (perBlock) hipLaunchKernelGGL(k_cos_block, dim3((unsigned)((B * nbx * nby + 3) / 4)), dim3(256), 0, stream, D, B, nbx, nby, dP, feats, cosPool);
        else hipLaunchKernelGGL(k_cos_wave, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, D, B, dP, feats, cosPool);
        return hipGetLastError();
    }
    {
        // a few problems of larger maps (the single-pair call: 200 x 200 objects = 169 blocks): one wave per 16 x 16 block as well, eight
        // chunks of loads in flight per wave — the tile kernel below gives such a call sixteen workgroups with two stages in flight
        // (29 us; the contraction over the descriptor is serial either way).  Up to eight waves per compute unit; !sw.cos_block_large: never
        const int nbx = (maxN1 + 15) / 16, nby = (maxN2 + 15) / 16;
        if (sw.cos_block_large && (int64_t)B * nbx * nby <= 8 * (int64_t)c->num_cu) {
            hipLaunchKernelGGL(k_cos_block, dim3((unsigned)((B * nbx * nby + 3) / 4)), dim3(256), 0, stream, D, B, nbx, nby, dP, feats, cosPool);
            return hipGetLastError();
        }
    }
    auto tiles = [](int n) { return (((n + 15) >> 4) + 3) >> 2; };     // cos_tiles()
    const int G = tiles(maxN1) * tiles(maxN2);
    const size_t lds = (size_t)2 * 128 * (COS_KC * 8 + 16);
    const hipError_t e = dyn_lds(c, reinterpret_cast<const void*>(k_cos_tile), lds);
    if (e != hipSuccess) return e;
    // one workgroup per tile, all tiles of a problem on one XCD: whole groups of eight problems
    hipLaunchKernelGGL(k_cos_tile, dim3((unsigned)(G * ((B + 7) / 8) * 8)), dim3(256), lds, stream, D, B, G, dP, feats, cosPool);
    return hipGetLastError();
}

// smallOut != NULL (batch calls: score and solve in one go): problems of the reference's demo scale (<= SMALL_MAXL live
// associations) are finished by k_small right behind the live lists — tests, positions, values, solve, pose in one kernel —
// and pass the rest of the sequence by.  The stepwise entry points (roman_score, then roman_solve / the export calls) keep
// the general layout for every problem.
int enqueue_score(roman_ctx* c, const DevParams& Din, const roman_params_t* params, const BatchIn& in, std::vector<ProbDesc>& hd, DevParams* Dout,
                  const BatchOut* smallOut = nullptr, const double* smallU0 = nullptr, bool mno = false /* roman_mno_batch*: every problem in the stream layout */)
{
    const Switches sw = read_switches();
    const int B = in.B;
    hd.assign(B, ProbDesc{});
    int64_t sumA = 0, sumCos = 0, sumTab = 0, sumQ4 = 0;
    int maxN12 = 0, maxN = 0, maxA = 0, maxN1 = 0, maxN2 = 0; int64_t maxTab = 0, poolRows = 0 /* rows of the feature pool the batch names */;
    bool allToAll = true;                              // no problem carries an explicit association list (k_cos_live's condition)
    for (int b = 0; b < B; ++b) {
        ProbDesc& d = hd[b];
        d.off1 = in.off1[b]; d.off2 = in.off2[b]; d.n1 = in.n1[b]; d.n2 = in.n2[b];
        if (d.n1 < 0 || d.n2 < 0) return fail(c, ROMAN_E_INVALID, "negative map size in problem %d", b);
        const int64_t na_list = in.assoc ? in.assoc_off[b + 1] - in.assoc_off[b] : 0;
        if (in.assoc && (na_list < 0 || na_list > 2147483647LL || in.assoc_off[b] < 0)) return fail(c, ROMAN_E_INVALID, "bad assoc_off at problem %d", b);
        if (in.assoc && na_list > 0) {
            d.assocOff = in.assoc_off[b];
            d.nA = (int32_t)na_list;
            allToAll = false;
        } else {                                       // no list, or an EMPTY one: all-to-all (clipperpy replaces an empty A likewise)
            d.assocOff = -1;
            const int64_t na = (int64_t)d.n1 * d.n2;
            if (na > 2147483647LL) return fail(c, ROMAN_E_TOO_LARGE, "n1*n2 overflows int32 in problem %d", b);
            d.nA = (int32_t)na;
        }
        d.liveOff = sumA; d.cosOff = sumCos; d.tabOff = sumTab; d.normOff = 0;
        if (sumQ4 > 2147483647LL) return fail(c, ROMAN_E_TOO_LARGE, "the tables of this batch exceed the bin pool's 32-bit offsets; split it");
        d.qtabOff4 = (int32_t)sumQ4;
        sumQ4 += ((int64_t)d.n1 * ((d.n1 + 3) & ~3) + (int64_t)d.n2 * ((d.n2 + 3) & ~3)) / 4;
        maxA = std::max(maxA, d.nA);
        sumA += d.nA; sumCos += (int64_t)d.n1 * d.n2; sumTab += (int64_t)d.n1 * d.n1 + (int64_t)d.n2 * d.n2;
        maxN12 = std::max(maxN12, d.n1 + d.n2); maxN = std::max(maxN, std::max(d.n1, d.n2));
        maxN1 = std::max(maxN1, d.n1); maxN2 = std::max(maxN2, d.n2);
        maxTab = std::max(maxTab, (int64_t)d.n1 * d.n1 + (int64_t)d.n2 * d.n2);
        poolRows = std::max(poolRows, std::max(d.off1 + d.n1, d.off2 + d.n2));
    }
    if (sumA > 2000000000LL) return fail(c, ROMAN_E_TOO_LARGE, "batch has %lld associations; split it (limit 2e9 per call)", (long long)sumA);
    const size_t nA1 = (size_t)std::max<int64_t>(sumA, 1);
    DevParams D = Din;
    const bool cosOn = D.p.cos_feature_dim > 0;

    Sizing SZ;
    estimate_sizes(c, sw, D, params, in.F, hd, &SZ);
    // a workspace never shrinks: keep what earlier (larger) batches made it hold
    SZ.capMaskWords = std::max(SZ.capMaskWords, WS.capMaskWords); SZ.capNnz = std::max(SZ.capNnz, WS.capNnz); SZ.capList = std::max(SZ.capList, WS.capList);
    // stream layout: as many live associations as the LDS tiles of this launch are sized for
    D.stream_maxL = std::min(STREAM_MAXL, std::max(64, (SZ.expectMaxL + 63) & ~63));
    // The fallback layout's kernels (symmetric SELL fill, k_solve / k_solve_wide) are launched only when a problem can
    // need them: no history yet, a live set beyond the stream layout expected, or parameters only k_solve handles.  Else a
    // problem that turns out too large for the LDS tiles of this launch is skipped (ROMAN_ST_WORKSPACE) and, the
    // history corrected, takes them on its second run.
    D.allow_fallback = (!c->hist.valid || SZ.expectMaxL > D.stream_maxL || D.p.maxiniters < 1 || D.p.maxlsiters < 1) ? 1 : 0;
    if (mno) {                                             // the mask rewrites the stream layout's values: every problem takes it (the caller has checked the list lengths)
        D.stream_maxL = std::min(STREAM_MAXL, std::max(64, (maxA + 63) & ~63));
        D.allow_fallback = 0;
    }
    {   // Which solver takes the fallback problems: few (large) ones -> k_solve_wide, every compute unit on one problem at a
        // time; many -> k_solve, one workgroup per problem.  Decided here because the fill writes 16-bit column labels for
        // the wide solver when every position fits (10 instead of 12 bytes per entry of the stream it is bound by).
        // (sw.wide: never / whenever a fallback problem can exist)
        const int mayFb = may_fallback(D, hd);
        // (many fallback problems: the teams take them when their live sets are KNOWN to be large — every association live (no single
        //  scores to remove any), or this parameter block's history says so; the first call of a gated method, whose live sets are a
        //  guess, keeps k_solve as its catch-all: no cooperative launch on the headline path)
        const bool bigLiveSets = !(D.single && !D.keep_all) || c->hist.valid;
        D.wide = (c->coop_ok && mayFb > 0 && D.p.maxiniters >= 1 && D.p.maxlsiters >= 1 && maxA <= (int64_t)WIDE_KW * c->num_cu * WIDE_NW * 64 &&
                  (sw.wide != CHOICE_LIB ? sw.wide == 1 : (mayFb <= std::max(1, c->num_cu / 4) || (bigLiveSets && SZ.expectMaxL >= 4608)))) ? 1 : 0;   // (several: teams of compute units, one problem each;
                  // measured, solve stage: 128 x L = 3 600 k_solve 10.7 ms / teams 12.9; 128 x L = 4 900 29 / ~24; 128 x L = 6 400 41.6 / 31.3; 96 x L = 10 000 118 / 63)
        D.idx16 = (D.wide && maxA <= 65534 && sw.wide_idx16) ? 1 : 0;                 // (!sw.wide_idx16: 32-bit labels always — tests)
    }
    *Dout = D;

    HIPCHK(c, WS.probs.ensure(sizeof(ProbDesc) * (size_t)B));
    HIPCHK(c, WS.state.ensure(sizeof(ProbState) * (size_t)B));
    HIPCHK(c, WS.totals.ensure(sizeof(BatchTotals)));
    HIPCHK(c, WS.queue.ensure(sizeof(int) * 16));              // [0..7]: the solvers' queues (k_skipped clears them), [8]: k_small's
    HIPCHK(c, WS.cosPool.ensure(sizeof(double) * (size_t)(cosOn ? std::max<int64_t>(sumCos, 1) : 1)));
    HIPCHK(c, WS.tabPool.ensure(sizeof(double) * (size_t)std::max<int64_t>(sumTab, 1)));
    HIPCHK(c, WS.sTmp.ensure(sizeof(double) * nA1));
    {
        DevBuf* i32s[] = {&WS.lp, &WS.li, &WS.lj, &WS.plp, &WS.pli, &WS.plj, &WS.rowCnt, &WS.rowPos, &WS.perm, &WS.sliceWidth, &WS.sliceBase, &WS.listOff};
        for (DevBuf* b_ : i32s) HIPCHK(c, b_->ensure(sizeof(int32_t) * nA1));
        DevBuf* f64s[] = {&WS.ls, &WS.ld, &WS.lza, &WS.lzb, &WS.pls, &WS.pld, &WS.plza, &WS.plzb};
        for (DevBuf* b_ : f64s) HIPCHK(c, b_->ensure(sizeof(double) * nA1));
    }
    HIPCHK(c, WS.maskPool.ensure(sizeof(unsigned long long) * (size_t)SZ.capMaskWords));
    HIPCHK(c, WS.listPool.ensure(sizeof(uint16_t) * (size_t)std::max<long long>(SZ.capList, 4)));
    HIPCHK(c, WS.prefPool.ensure(sizeof(uint32_t) * (size_t)SZ.capMaskWords));
    HIPCHK(c, WS.vals.ensure(sizeof(double) * (size_t)SZ.capNnz));
    HIPCHK(c, WS.cols16.ensure(sizeof(uint16_t) * (size_t)SZ.capNnz));
    HIPCHK(c, WS.cols32.ensure(sizeof(uint32_t) * (size_t)SZ.capNnz));
    WS.capMaskWords = SZ.capMaskWords; WS.capNnz = SZ.capNnz; WS.capList = SZ.capList;
    // work items: blocks of RPB consecutive live rows of one problem (more, smaller items for small batches)
    int RPB = 32;
    while (RPB < 128 && (int64_t)RPB * c->num_cu * 64 < sumA) RPB <<= 1;     // 128: ~17 items per problem balance the static item loop best (measured 32..1024)
    const size_t maxItems = (size_t)(sumA / RPB) + (size_t)B + 1;
    HIPCHK(c, WS.items.ensure(sizeof(ItemDesc) * maxItems));

    {   // descriptors: through pinned staging
        ProbDesc* staged = nullptr;
        HIPCHK(c, WS.probStage.stage((size_t)B, &staged));
        memcpy(staged, hd.data(), sizeof(ProbDesc) * (size_t)B);
        HIPCHK(c, WS.probStage.upload(WS.probs, (size_t)B, WS.stream));
    }
    const ProbDesc* dP = WS.probs.as<ProbDesc>();
    ProbState* dS = WS.state.as<ProbState>();
    BatchTotals* dT = WS.totals.as<BatchTotals>();
    const LivePools LP{WS.lp.as<int32_t>(), WS.li.as<int32_t>(), WS.lj.as<int32_t>(), WS.ls.as<double>(), WS.ld.as<double>(), WS.lza.as<double>(), WS.lzb.as<double>()};
    const LivePools PP{WS.plp.as<int32_t>(), WS.pli.as<int32_t>(), WS.plj.as<int32_t>(), WS.pls.as<double>(), WS.pld.as<double>(), WS.plza.as<double>(), WS.plzb.as<double>()};

    StageTimer t0(c, ROMAN_STAGE_SINGLE);
    bool cosScreen = false, cosLive = false;           // cosLive: k_cos_live has scored the problems it did not flag, k_live takes the flagged ones
    if (cosOn && maxN1 > 0 && maxN2 > 0) {
        cosScreen = cos_sel_applies(c, sw, D, B, maxN1, maxN2, poolRows);
        ++(cosScreen ? c->cosScreenBatches : c->cosDenseBatches);
        if (cosScreen) {
            HIPCHK(c, WS.cosDense.ensure(sizeof(int32_t) * (size_t)B));
            cosLive = allToAll && !D.keep_all && !D.plain_all;
            if (cosLive)
                HIPCHK(c, launch_cos_live(c, WS.stream, D, B, maxN1, maxN2, dP, in.feats, WS.cosPool.as<double>(), WS.cosDense.as<int32_t>(), dS, LP));
            else
                HIPCHK(c, launch_cos_sel(c, WS.stream, D, B, maxN1, maxN2, dP, in.feats, WS.cosPool.as<double>(), WS.cosDense.as<int32_t>(), false));
        } else
        HIPCHK(c, launch_cos(c, sw, WS.stream, D, B, maxN1, maxN2, dP, in.feats, WS.cosPool.as<double>()));
    DBG(c, "k_cos");
    }
    if (maxTab > 0) {
        const size_t tabLds = sizeof(double) * 3 * (size_t)std::max(maxN, 1);
        if (tabLds > c->lds_max) return fail(c, ROMAN_E_TOO_LARGE, "maps of %d objects exceed the LDS point staging of this build", maxN);
        HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(k_tables), tabLds));
        // bands: enough workgroups to fill the device twice, no more (every band stages the whole map's points)
        const int bands = std::max(1, std::min((maxN + 15) / 16, (2 * c->num_cu + 2 * B - 1) / (2 * B)));
        const int RBt = (((maxN + bands - 1) / bands) + 15) & ~15;
        const int thr = RBt >= 64 ? 1024 : 256;
        // (the same entries as 15-bit bins for k_count's prefilter: 2 more bytes per entry)
        uint16_t* qtab = nullptr;
        if (D.pre_invw > 0.0 && std::isfinite(D.pre_invw)) {
            HIPCHK(c, WS.qtabPool.ensure(sizeof(uint16_t) * 4 * (size_t)std::max<int64_t>(sumQ4, 1) + 64));
            qtab = WS.qtabPool.as<uint16_t>();
        }
        hipLaunchKernelGGL(k_tables, dim3((unsigned)((maxN + RBt - 1) / RBt), 2, B), dim3(thr), tabLds, WS.stream, D, dP, in.feats, WS.tabPool.as<double>(), RBt, qtab);
    DBG(c, "k_tables");
    }
    {   // single scores, then the ordered compaction of the live associations: chunks x problems (behind k_cos_live: its flagged problems only)
        const int maxChunks = std::max(1, (maxA + LIVE_CHUNK - 1) / LIVE_CHUNK);
        const int32_t* only = cosLive ? WS.cosDense.as<int32_t>() : nullptr;
        HIPCHK(c, WS.chunkCnt.ensure(sizeof(int32_t) * (size_t)B * (size_t)maxChunks * 4));      // live associations per wave segment
        hipLaunchKernelGGL(k_live<0>, dim3((unsigned)maxChunks, (unsigned)B), dim3(256), 0, WS.stream, D, dP, dS, in.feats, in.assoc, WS.cosPool.as<double>(), WS.sTmp.as<double>(), PP.lp /* scratch until k_upper */,
                           WS.chunkCnt.as<int32_t>(), maxChunks, LP.lp, LP.li, LP.lj, LP.ls, LP.ld, LP.lza, LP.lzb, only);
        hipLaunchKernelGGL(k_live<1>, dim3((unsigned)maxChunks, (unsigned)B), dim3(256), 0, WS.stream, D, dP, dS, in.feats, in.assoc, WS.cosPool.as<double>(), WS.sTmp.as<double>(), PP.lp /* scratch until k_upper */,
                           WS.chunkCnt.as<int32_t>(), maxChunks, LP.lp, LP.li, LP.lj, LP.ls, LP.ld, LP.lza, LP.lzb, only);
    DBG(c, "k_live");
    }
    t0.stop();

    // pair-test kernel LDS: a column tile (objects [+ z] of every live association) + per wave the table rows of
    // the NR rows it sweeps together (NR = 2 if that fits beside the whole column tile, else 1).  The tile is sized
    // for the EXPECTED largest live set; a problem that exceeds it reads its columns from memory instead.
    const int expL = std::max(SZ.expectMaxL, 1);
    const int ldsPerRow = ((2 * std::max(maxN, 1) + 1 + 1) & ~1) + 2;     // n1 + sentinel + n2 doubles
    const int colBytesC = D.gravity ? 20 : 4;                             // [z pair] + packed 16-bit table-slice indices
    const int Lneed = (expL + 255) & ~255;
    // (two rows per wave when their table slices leave room for the whole expected live set — or, for live sets beyond any
    //  tile, for a tile of at least 2048 columns: k_count sweeps larger live sets tile by tile)
    const int NRc = ((size_t)16 * 2 * ldsPerRow * sizeof(double) + (size_t)std::min(Lneed, 2048) * colBytesC <= c->lds_max) ? 2 : 1;
    int wpb = 16;
    while (wpb > 1 && (size_t)wpb * NRc * ldsPerRow * sizeof(double) + 256 * colBytesC > c->lds_max) wpb >>= 1;
    if ((size_t)wpb * NRc * ldsPerRow * sizeof(double) + 256 * colBytesC > c->lds_max)
        return fail(c, ROMAN_E_TOO_LARGE, "maps of %d objects exceed the LDS table staging of this build", maxN);
    const int ldsPerWave = NRc * ldsPerRow;
    const size_t tabLds = (size_t)wpb * ldsPerWave * sizeof(double);
    int TCc = (int)std::min<size_t>((c->lds_max - tabLds) / colBytesC, 32768) & ~255;
    TCc = std::min(TCc, Lneed);
    const size_t pairLds = tabLds + (size_t)TCc * colBytesC;
    const int pairGrid = c->num_cu * std::max(1, std::min(2048 / (wpb * 64), (int)(c->lds_max / pairLds)));
    // The one-tile sweep with candidate generation in front of the exact gate (count_rows_pre, round 6): column tile without the z
    // pairs (the exact gate reads them per object: from a table in LDS sized at the launch, or from memory) + per wave the table slices, their
    // 16-bit bin slices, the candidate queue and the rows' mask words.  Taken when the whole expected live set fits its tile;
    // sw.count_pre forces the plain sweep / the prefilter where it fits (A/B and tests).
    int preNR = 0, preWpb = 0, preTC = 0; size_t preLds = 0;
    const int preRow = (2 * std::max(maxN, 1) + 1 + 3) & ~3;                 // entries of the packed bin table (n1 + sentinel + n2)
    {
        const bool want = sw.count_pre != 0 && D.pre_invw > 0.0 && std::isfinite(D.pre_invw) && Lneed <= (sw.count_pre != CHOICE_LIB ? 16000 : 4096) && maxN <= 32767;   // (live sets beyond the stream layout's: measured slower there — 64 x L = 10 000: 5.8 against 4.0 ms with the tiled plain sweep; forced on by ROMAN_COUNT_PRE=1 up to 16 000)
        if (want) {
            const int tc = Lneed;
            for (int wp = PRE_WAVES; wp >= 8; wp -= 4) {
                const size_t need = (size_t)(tc + PRE_COLPAD + 4) * 4 + (size_t)wp * (size_t)count_pre_wave_bytes(preRow, tc);
                if (need <= c->lds_max) { preNR = PRE_NR; preWpb = wp; preTC = tc; preLds = need; break; }
            }
        }
    }

    StageTimer t1(c, ROMAN_STAGE_COUNT_PASS);                  // (the stage also holds k_small: at the demo scale it IS the rest of the alignment)
    {   // demo-scale problems: finished here, in one kernel (k_small); launched when such problems have been seen with this
        // parameter block (or, with no history yet, when the association lists are short enough to make them likely)
        const bool want = smallOut != nullptr && sw.small_fused /* off: never (A/B) */ && D.p.maxiniters >= 1 && D.p.maxlsiters >= 1 && maxTab > 0 &&
                          (c->hist.valid ? c->hist.smallSeen : maxA <= 16 * SMALL_MAXL);
        if (want) {
            SolveOut O;
            int rc = make_solve_out(c, B, sumA, *smallOut, &O);
            if (rc) return rc;
            HIPCHK(c, hipMemsetAsync(WS.queue.as<int>() + 8, 0, sizeof(int), WS.stream));
            const bool fast = D.single && (D.p.single_mode == ROMAN_SINGLE_BOTH || D.p.single_mode == ROMAN_SINGLE_OFFDIAG) && D.p.distance_weight == 1.0 &&
                              D.p.fusion_method != ROMAN_FUSE_ARITHMETIC_MEAN && D.p.fusion_method != ROMAN_FUSE_PRODUCT;      // (k_fill_list's own choice)
            constexpr size_t ldsSmall = small_lds_bytes();     // 3 vectors of 192 + reduction scratch + coordinate list + the problem's columns (~14 KB)
            const int grid = std::max(1, std::min(B, c->num_cu * 12));
            auto ks = fast ? k_small<true> : k_small<false>;
            hipLaunchKernelGGL(ks, dim3(grid), dim3(64), ldsSmall, WS.stream, D, B, dP, dS, in.feats, in.assoc, WS.tabPool.as<double>(),
                               LP.lp, LP.li, LP.lj, LP.ls, LP.ld, LP.lza, LP.lzb, WS.plp.as<int32_t>(), WS.pld.as<double>(), WS.rowPos.as<uint32_t>(),
                               smallU0, O, WS.queue.as<int>() + 8);
    DBG(c, "k_small");
            // Every problem of this parameter block has so far been finished by k_small: the general kernels (twelve launches
            // that would find nothing to do: ~0.25 ms per call of 4096 problems) are left out.  A problem k_small leaves behind
            // is then skipped like a workspace overflow (ROMAN_ST_WORKSPACE) and the history remembers that they are needed.
            D.small_only = (c->hist.valid && !c->hist.generalSeen && sw.small_only /* off: never leave them out */) ? 1 : 0;
            Dout->small_only = D.small_only;
        }
    }
    hipLaunchKernelGGL(k_rowbase, dim3(1), dim3(B > 256 ? 1024 : 256), 0, WS.stream, B, RPB, SZ.capMaskWords, dS, dT, D.small_only, cosScreen ? (const int32_t*)WS.cosDense.as<int32_t>() : (const int32_t*)nullptr);
    DBG(c, "k_rowbase");
    if (!D.small_only) {
    hipLaunchKernelGGL(k_items, dim3(B), dim3(256), 0, WS.stream, RPB, dS, WS.items.as<ItemDesc>());
    DBG(c, "k_items");
    }
    if (sumA > 0 && !D.small_only) {
        // two instantiations over the same items: the one-tile sweep for live sets that fit the LDS column tile, and — launched
        // only when such problems can exist (fallback problems, or a tile capped by the LDS) — the tile-by-tile sweep for the rest
        const bool needTiled = D.allow_fallback || TCc < Lneed;
        int degGiven = 0;
        for (int tiled = 0; tiled < (needTiled ? 2 : 1); ++tiled) {
            const void* kc = nullptr;
#define ROMAN_KC(GM_) kc = tiled ? (NRc == 2 ? reinterpret_cast<const void*>(k_count<GM_, 2, true>) : reinterpret_cast<const void*>(k_count<GM_, 1, true>)) \
                                 : (NRc == 2 ? reinterpret_cast<const void*>(k_count<GM_, 2, false>) : reinterpret_cast<const void*>(k_count<GM_, 1, false>))
            switch (D.gmode) { case 1: ROMAN_KC(1); break; case 2: ROMAN_KC(2); break; case 3: ROMAN_KC(3); break; default: ROMAN_KC(0); break; }
#undef ROMAN_KC
            const bool usePre = !tiled && preNR > 0;
            if (usePre) {
#define ROMAN_KP(GM_) kc = reinterpret_cast<const void*>(k_count<GM_, 1, false, true>)
                switch (D.gmode) { case 1: ROMAN_KP(1); break; case 2: ROMAN_KP(2); break; case 3: ROMAN_KP(3); break; default: ROMAN_KP(0); break; }
#undef ROMAN_KP
            }
            const size_t ldsK = usePre ? preLds : pairLds;
            const int wpbK = usePre ? preWpb : wpb;
            const int gridK = usePre ? c->num_cu * std::max(1, std::min(2048 / (wpbK * 64), (int)(c->lds_max / ldsK))) : pairGrid;
            // (the prefiltered sweep of a batch with at least a problem per compute unit takes whole problems as work items: RPB = -B;
            //  sw.count_whole forces the row blocks / whole problems; + the rows' degrees in LDS then)
            const bool wholeP = usePre && (sw.count_whole != CHOICE_LIB ? sw.count_whole == 1 : B >= c->num_cu) && preLds + (size_t)preTC * 4 <= c->lds_max;
            if (wholeP) degGiven = 1;                            // k_count counts the degrees as the pairs pass: k_lists skips its degree sweep
            // (the prefiltered sweep's exact gate takes the heights of a candidate's two objects from a per-object table in LDS, one
            //  double per entry of the packed bin table, where that fits without costing a resident workgroup; from memory otherwise:
            //  !sw.count_zlds forces the memory path, which maps near the LDS limit take — tests)
            size_t ldsLaunch = ldsK + (wholeP ? (size_t)preTC * 4 : 0);
            const size_t zBytes = (size_t)preRow * sizeof(double);
            const bool zLds = usePre && D.gmode != 0 && sw.count_zlds && ldsLaunch + zBytes <= c->lds_max &&
                              c->lds_max / (ldsLaunch + zBytes) >= std::min<size_t>(gridK / c->num_cu, c->lds_max / ldsLaunch);
            if (zLds) ldsLaunch += zBytes;
            HIPCHK(c, dyn_lds(c, kc, ldsLaunch));
            DevParams a_D = D; const ProbDesc* a_dP = dP; const ProbState* a_dS = dS; const BatchTotals* a_dT = dT; const ItemDesc* a_items = WS.items.as<ItemDesc>();
            const double* a_tab = WS.tabPool.as<double>(); const int32_t* a_li = LP.li; const int32_t* a_lj = LP.lj; const double* a_za = LP.lza; const double* a_zb = LP.lzb;
            uint32_t* a_rc = WS.rowCnt.as<uint32_t>(); unsigned long long* a_mask = WS.maskPool.as<unsigned long long>(); uint32_t* a_pref = WS.prefPool.as<uint32_t>();
            int a_TC = usePre ? preTC : TCc, a_lpw = usePre ? preRow : ldsPerWave;
            int a_RPB = wholeP ? -B : RPB;
            const uint16_t* a_qtab = WS.qtabPool.as<uint16_t>();
            int a_zLds = zLds ? 1 : 0;
            void* args[] = {&a_D, &a_dP, &a_dS, &a_dT, &a_items, &a_tab, &a_li, &a_lj, &a_za, &a_zb, &a_rc, &a_mask, &a_pref, &a_TC, &a_lpw, &a_RPB, &a_qtab, &a_zLds};
            HIPCHK(c, hipLaunchKernel(kc, dim3(gridK), dim3(wpbK * 64), args, ldsLaunch, WS.stream));
        }
    DBG(c, "k_count");
        // Stream-layout problems (kind 0) go from the upper blocks straight to positions and kept-candidate lists in ONE kernel, one
        // workgroup per problem (k_lists, round 5); the symmetric matrix and its four kernels remain for the fallback layout's
        // problems — launched only when such problems can occur — and, with sw.lists forced off, for everything (A/B).
        // (a handful of problems — the single-pair call — keep the four kernels: they spread ONE problem over the device, k_lists
        //  gives it one compute unit: 0.59 against 0.66 ms for B = 1)
        const int fusedLists = sw.lists != CHOICE_LIB ? sw.lists : (B >= std::max(8, c->num_cu / 8) ? 1 : 0);      // (sw.lists: never / always — A/B and tests)
        if (fusedLists) {
            // The LDS the kernel leaves (~83 KB of 160: one workgroup per compute unit either way, by its registers) holds the window of
            // list entries it builds in place and writes out in whole quads; entries beyond it are stored where they go, one at a time.
            // sw.lists_lds = n: a window of n bytes instead (0: none — every entry stored on its own, A/B).
            // Probe of round 6: behind the prefiltered k_count with whole problems as work items k_lists takes 162-165 us in some
            // processes and 192-210 us in others (every launch of a process alike; identical instruction and byte counters,
            // SQ_WAIT_INST_ANY 122 M -> 190-220 M wave-cycles; behind the plain sweep or row-block work items always 160-169 us).  NOT the
            // cause, each measured with a throw-away build (tools/r6_lists_probe.sh is the per-process probe): two workgroups on one compute unit (an LDS pad), which workgroup takes which
            // problem (rotations by 1, 4, 8, 128), dirty mask lines in L2 (non-temporal stores: -3 us).  Open.
            static size_t listsStatic = 0;
            if (listsStatic == 0) {
                hipFuncAttributes fa;
                HIPCHK(c, hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_lists)));
                listsStatic = std::max<size_t>(fa.sharedSizeBytes, 1);
            }
            const size_t room = c->lds_max > listsStatic ? c->lds_max - listsStatic : 0;
            const size_t winBytes = std::min(room, sw.lists_lds >= 0 ? (size_t)sw.lists_lds : room) & ~(size_t)15;
            if (winBytes) HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(k_lists), winBytes));
            hipLaunchKernelGGL(k_lists, dim3((unsigned)std::max(1, std::min(B, 2 * c->num_cu))), dim3(LISTS_NT), winBytes, WS.stream, B, dP, dS, dT,
                               WS.maskPool.as<unsigned long long>(), WS.listPool.as<uint16_t>(), WS.listOff.as<uint32_t>(),
                               WS.rowCnt.as<uint32_t>(), WS.perm.as<uint32_t>(), WS.rowPos.as<uint32_t>(), LP, PP, (long long)SZ.capList, sw.sort_eq_max, degGiven,
                               (int)(winBytes / sizeof(uint16_t)));
    DBG(c, "k_lists");
        }
        if (!fusedLists || D.allow_fallback) {
        {   // lower triangle of the bit matrices = transposed blocks of the upper triangle (grid for the expected size;
            // the kernel loops when a problem is larger)
            const int Wexp = (expL + 63) / 64;
            const int tasks = ((Wexp + 7) / 8) * ((std::max(Wexp - 1, 1) + 7) / 8);          // workgroups of 8 waves
            const int T = std::max(tasks, 1);
            hipLaunchKernelGGL(k_mirror, dim3((unsigned)(T * ((B + 7) / 8) * 8)), dim3(512), 0, WS.stream, B, T, dS, WS.maskPool.as<unsigned long long>(), fusedLists);
    DBG(c, "k_mirror");
        }
        hipLaunchKernelGGL(k_rowprefix, dim3(c->num_cu * 2), dim3(1024), 0, WS.stream, dP, dS, dT, WS.items.as<ItemDesc>(),
                           WS.maskPool.as<unsigned long long>(), WS.prefPool.as<uint32_t>(), WS.rowCnt.as<uint32_t>(), RPB, fusedLists);
    DBG(c, "k_rowprefix");
        // the stream layout's bitonic sort takes N/2 threads for N = 2^k >= L keys; the fallback layout's counting sort is written
        // for 1024 (at the reference's demo scale — 60 live associations — 4096 workgroups of 1024 threads were 99 us of a 1.4 ms call)
        int sortThr = 1024;
        if (!D.allow_fallback) { int N2 = 64; while (N2 < expL) N2 <<= 1; sortThr = std::max(64, std::min(1024, N2 / 2)); }
        hipLaunchKernelGGL(k_rowsort, dim3(B), dim3(sortThr), 0, WS.stream, dP, dS, dT, WS.rowCnt.as<uint32_t>(), WS.rowPos.as<uint32_t>(), WS.perm.as<uint32_t>(),
                           WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.listOff.as<uint32_t>(), SZ.capList, fusedLists, sw.sort_eq_max);
    DBG(c, "k_rowsort");
        if (!fusedLists) {
        // small live sets (the reference's demo scale): a work item is a whole problem of a few dozen rows — more, smaller
        // workgroups keep more of them in flight (a row is a chain of dependent memory round trips)
        const int upThr = expL <= 256 ? 256 : 1024;
        hipLaunchKernelGGL(k_upper, dim3(c->num_cu * 2 * (1024 / upThr)), dim3(upThr), 0, WS.stream, dP, dS, dT, WS.items.as<ItemDesc>(),
                           WS.maskPool.as<unsigned long long>(), WS.listPool.as<uint16_t>(), WS.listOff.as<uint32_t>(),
                           WS.rowCnt.as<uint32_t>(), WS.perm.as<uint32_t>(), WS.rowPos.as<uint32_t>(), LP, PP, RPB);
    DBG(c, "k_upper");
        }
        }
        hipLaunchKernelGGL(k_slicegeom, dim3(B), dim3(64), 0, WS.stream, dP, dS, WS.rowCnt.as<uint32_t>(), WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>());
    DBG(c, "k_slicegeom");
    }
    // k_fill_list work items: groups of consecutive slices of one problem, about 3 per CU for the whole batch
    // (about 3 groups per CU, EVERY problem cut into the same number NG of groups: the static deal of the groups to the
    // workgroups then gives each one heavy (first slices) and two light groups; whole problems per workgroup or cuts
    // that differ between problems measured 0.46-0.63 ms against 0.38-0.40)
    int NG = (int)std::max<int64_t>(1, std::min<int64_t>(FILLS_MAXSPI, (3 * (int64_t)c->num_cu + B / 2) / std::max(B, 1)));
    {   // a workgroup takes every (grid/8)-th group of its XCD's range: the residues it meets (which part of a problem
        // a group is) rotate through all NG values only if that stride is coprime to NG — NG = 4 on 256 CUs (stride 32)
        // hands some workgroups nothing but first, heavy groups (fill 0.59 ms against 0.38 with NG = 3)
        const int stride = std::max(1, (c->num_cu & ~7) / 8);
        auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
        while (NG > 1 && gcd(stride % NG, NG) != 1) --NG;
    }
    const int Wmax = std::max(1, D.stream_maxL / 64);
    const int SPI = (Wmax + std::min(NG, Wmax) - 1) / std::min(NG, Wmax);       // slices per group at most (LDS capacity)
    if (!D.small_only) {
    hipLaunchKernelGGL(k_probscan, dim3(1), dim3(B > 256 ? 1024 : 256), 0, WS.stream, B, NG, SZ.capNnz, dS, dT);
    DBG(c, "k_probscan");
    }
    t1.stop();

    StageTimer t2(c, ROMAN_STAGE_FILL);
    if (sumA > 0 && !D.small_only) {
        // list fill (stream layout): column tile + the rows and slice tables of one group
        const int colBytesF = D.gravity ? 32 : 16;
        const int TCs = D.stream_maxL;
        // the objects' coordinates in LDS (32 bytes per object) instead of the z columns, when they fit: the fill then
        // recomputes the distances instead of gathering them from the tables
        const int NO = (std::max(maxN, 1) + 1) & ~1;
        const size_t groupLds = sizeof(uint32_t) * (size_t)(3 * SPI * 64 + 2 * (SPI + 1) + 4 * FILL_WIN + 1 + 2);    // (+ the window's mask / slice / prefix tables)
        const bool obj = (size_t)TCs * (16 + 2) + (size_t)64 * NO + groupLds <= c->lds_max;
        const size_t sliceLds = obj ? (size_t)TCs * (16 + 2) + (size_t)64 * NO + groupLds : (size_t)TCs * (colBytesF + 2) + groupLds;
        if (sliceLds > c->lds_max) return fail(c, ROMAN_E_TOO_LARGE, "internal: stream column tile does not fit the LDS");
        const bool fast = D.single && (D.p.single_mode == ROMAN_SINGLE_BOTH || D.p.single_mode == ROMAN_SINGLE_OFFDIAG) && D.p.distance_weight == 1.0 &&
                          D.p.fusion_method != ROMAN_FUSE_ARITHMETIC_MEAN && D.p.fusion_method != ROMAN_FUSE_PRODUCT;
        auto kf = D.gravity ? (fast ? k_fill_list<true, true, false> : k_fill_list<true, false, false>) : (fast ? k_fill_list<false, true, false> : k_fill_list<false, false, false>);
        if (obj) kf = D.gravity ? (fast ? k_fill_list<true, true, true> : k_fill_list<true, false, true>) : (fast ? k_fill_list<false, true, true> : k_fill_list<false, false, true>);
        HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(kf), sliceLds));
        const int fillThr = expL <= 256 ? 256 : 1024;          // (k_upper: small problems, small workgroups, more of them)
        const int fillWgs = std::max(1, std::min(1024 / fillThr, (int)(c->lds_max / sliceLds)));
        hipLaunchKernelGGL(kf, dim3((unsigned)((c->num_cu & ~7) * fillWgs)), dim3(fillThr), sliceLds, WS.stream,
                           D, B, dP, dS, dT, WS.tabPool.as<double>(), in.feats, NO, LP.li, LP.lj, LP.ls, LP.lza, LP.lzb,
                           WS.listPool.as<uint16_t>(), WS.listOff.as<uint32_t>(), WS.rowCnt.as<uint32_t>(), WS.perm.as<uint32_t>(), WS.rowPos.as<uint32_t>(),
                           WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.cols16.as<uint16_t>(), WS.vals.as<double>(), TCs, NG, SPI);
    DBG(c, "k_fill_list");
        // fallback layout (symmetric SELL-64, 32-bit indices) for the problems the stream layout does not take: only when
        // one can exist (the kernel would find no work otherwise)
        if (D.allow_fallback && (SZ.maxA > D.stream_maxL || D.p.maxiniters < 1 || D.p.maxlsiters < 1)) {
            const int colBytesG = D.gravity ? 40 : 24;
            const size_t ringLds = (size_t)16 * 3 * FILL_Q * sizeof(uint32_t) + (size_t)FILL_RPB * FILL_ROWBYTES;     // per-wave rings + the item's rows
            static_assert(FILL_RPB >= 128, "the work items of a batch are blocks of at most 128 rows");
            int TCf = (int)std::min<size_t>((c->lds_max - ringLds) / colBytesG, 32768) & ~63;
            TCf = std::min(TCf, std::max(64, (Lneed + 63) & ~63));      // (a multiple of 64, at least 64: k_fill cuts larger live sets into windows of TCf columns)
            const size_t fillLds = ringLds + (size_t)TCf * colBytesG;
            const int fillGrid = c->num_cu * std::max(1, std::min(2, (int)(c->lds_max / fillLds)));
            if (D.idx16) {                                      // 16-bit column labels for k_solve_wide
                auto kg = D.gravity ? k_fill<true, uint16_t, true> : k_fill<false, uint16_t, true>;
                HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(kg), fillLds));
                hipLaunchKernelGGL(kg, dim3(fillGrid), dim3(1024), fillLds, WS.stream, D, dP, dS, dT, WS.items.as<ItemDesc>(), WS.tabPool.as<double>(),
                                   LP.li, LP.lj, LP.ls, LP.lza, LP.lzb,
                                   WS.rowCnt.as<uint32_t>(), WS.maskPool.as<unsigned long long>(), WS.prefPool.as<uint32_t>(), WS.rowPos.as<uint32_t>(),
                                   WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.cols16.as<uint16_t>(), WS.vals.as<double>(), TCf, RPB, (const uint32_t*)WS.perm.as<uint32_t>());
            } else {
                auto kg = D.gravity ? k_fill<true, uint32_t, true> : k_fill<false, uint32_t, true>;
                HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(kg), fillLds));
                hipLaunchKernelGGL(kg, dim3(fillGrid), dim3(1024), fillLds, WS.stream, D, dP, dS, dT, WS.items.as<ItemDesc>(), WS.tabPool.as<double>(),
                                   LP.li, LP.lj, LP.ls, LP.lza, LP.lzb,
                                   WS.rowCnt.as<uint32_t>(), WS.maskPool.as<unsigned long long>(), WS.prefPool.as<uint32_t>(), WS.rowPos.as<uint32_t>(),
                                   WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.cols32.as<uint32_t>(), WS.vals.as<double>(), TCf, RPB, (const uint32_t*)WS.perm.as<uint32_t>());
            }
    DBG(c, "k_fill");
        }
    }
    t2.stop();
    // the totals travel back on their own: whoever sizes a later batch picks them up once they have arrived
    HIPCHK(c, hipMemcpyAsync(WS.pinnedTotals, dT, sizeof(BatchTotals), hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipEventRecord(WS.totEvent, WS.stream));
    WS.totPending = true; WS.totMaskBound = SZ.maskBound; WS.totSumA = SZ.sumA; WS.totMaxA = SZ.maxA; WS.totEpoch = c->histEpoch;
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// Solver + rounding + pose on the matrices held by the workspace.  `feats` may be NULL (dense
// matrix problems have no points: the pose is skipped).  mayFallback: a problem of the fallback kind can exist.
int enqueue_solve(roman_ctx* c, const DevParams& D, int B, int64_t sumA, int64_t maxA /* longest association list */, const double* feats, const int32_t* assoc,
                  const double* u0, bool hascz, int mayFallback /* problems that can be of the fallback kind */, const BatchOut& out)
{
    const Switches sw = read_switches();
    const size_t R1 = (size_t)std::max<int64_t>(sumA, 1);
    SolveOut O;
    { int rc_ = make_solve_out(c, B, sumA, out, &O); if (rc_) return rc_; }
#ifdef ROMAN_SOLVE_TIMING
    HIPCHK(c, WS.hAux3.ensure(sizeof(unsigned long long) * 16 * (size_t)B));
    HIPCHK(c, hipMemsetAsync(WS.hAux3.p, 0, sizeof(unsigned long long) * 16 * (size_t)B, WS.stream));
    O.dbg = WS.hAux3.as<unsigned long long>();
#endif
    // stream solver: LDS = three vectors of Lc elements (Lc: whole slices of stream_maxL + the 64 dummy elements the
    // inert padding entries point at) + reduction scratch + slice table
    constexpr int NW = SOLVE_WAVES;
    const int Lc = STREAM_MAXL + 64;                            // (fixed: the kernel addresses the three vectors at compile-time distances)
    const size_t ldsUp = (size_t)3 * 8 * Lc + sizeof(double) * red_doubles(NW) + sizeof(uint32_t) * (ST_MAXSL + 2) + sizeof(int) * 8 + 16;
    const int wgPerCu = std::max(1, std::min((int)(c->lds_max / ldsUp), 2048 / (NW * 64)));
    const int gridUp = std::max(1, std::min(B, c->num_cu * wgPerCu));

    StageTimer t3(c, ROMAN_STAGE_SOLVE);
    const bool coopPlanned = mayFallback && D.wide != 0 && c->coop_ok;
    if (coopPlanned) {                                          // the whole-device solver's barrier words, problem queue and list (k_skipped fills the list)
        HIPCHK(c, WS.wideBar.ensure(sizeof(unsigned) * WIDE_BAR_WORDS));
        HIPCHK(c, WS.fbList.ensure(sizeof(int32_t) * (size_t)B));
        HIPCHK(c, hipMemsetAsync(WS.wideBar.p, 0, sizeof(unsigned) * WIDE_BAR_WORDS, WS.stream));      // counters, generations, queue and the abort flag start at 0 in every launch
    }
    hipLaunchKernelGGL(k_skipped, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, WS.stream, B, WS.probs.as<ProbDesc>(), WS.state.as<ProbState>(), O, WS.queue.as<int>(),
                       coopPlanned ? WS.fbList.as<int32_t>() : (int32_t*)nullptr, coopPlanned ? WS.wideBar.as<unsigned>() : (unsigned*)nullptr);
    DBG(c, "k_skipped");
    if (D.small_only) { t3.stop(); HIPCHK(c, hipGetLastError()); return ROMAN_OK; }   // every problem was k_small's (or is reported skipped)
    // Small problems (<= SMALL_MAXL live associations: the reference's demo scale) take the one-wave-per-problem
    // instantiation; it is launched when such problems have been seen with this parameter block (or, with no history
    // yet, when the association lists are short enough to make them likely).  The general launch takes the rest — and
    // everything when the small one is not part of the batch.
    const bool small = sw.small /* off: never */ && D.p.maxiniters >= 1 && D.p.maxlsiters >= 1 &&
                       (c->hist.valid ? c->hist.smallSeen : maxA <= 16 * SMALL_MAXL);
    const int Lc1 = SMALL_MAXL + 64;
    const size_t ldsUp1 = (size_t)3 * 8 * Lc1 + sizeof(double) * red_doubles(1) + sizeof(uint32_t) * (ST_MAXSL + 2) + sizeof(int) * 8 + 16 + (size_t)COO_CAP * 12;
    const int gridUp1 = std::max(1, std::min(B, c->num_cu * 24));
#define ROMAN_LAUNCH_UP(CZ_)                                                                                                  \
    do {                                                                                                                      \
        auto kup = k_solve_up<NW, CZ_, STREAM_MAXL>;                                                                          \
        HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(kup), ldsUp)); \
        hipLaunchKernelGGL(kup, dim3(gridUp), dim3(NW * 64), ldsUp, WS.stream, D, B, WS.probs.as<ProbDesc>(), WS.state.as<ProbState>(), feats, assoc, \
                           WS.plp.as<int32_t>(), WS.lp.as<int32_t>(), WS.rowPos.as<uint32_t>(), WS.pld.as<double>(), WS.sliceBase.as<uint32_t>(), \
                           WS.cols16.as<uint16_t>(), WS.vals.as<double>(), u0, O, WS.queue.as<int>(), Lc, small ? SMALL_MAXL + 1 : 0, STREAM_MAXL, (small && c->hist.valid && !c->hist.largeSeen) ? 64 : 1); \
        if (small) {                                                                                                          \
            HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(k_solve_up<1, CZ_, SMALL_MAXL>), ldsUp1));                       \
            hipLaunchKernelGGL((k_solve_up<1, CZ_, SMALL_MAXL>), dim3(gridUp1), dim3(64), ldsUp1, WS.stream, D, B, WS.probs.as<ProbDesc>(), WS.state.as<ProbState>(), feats, assoc, \
                               WS.plp.as<int32_t>(), WS.lp.as<int32_t>(), WS.rowPos.as<uint32_t>(), WS.pld.as<double>(), WS.sliceBase.as<uint32_t>(), \
                               WS.cols16.as<uint16_t>(), WS.vals.as<double>(), u0, O, WS.queue.as<int>() + 1, Lc1, 0, SMALL_MAXL, 1); \
        }                                                                                                                     \
    } while (0)
    if (hascz) ROMAN_LAUNCH_UP(true); else ROMAN_LAUNCH_UP(false);
#undef ROMAN_LAUNCH_UP
    DBG(c, "k_solve_up");
    if (mayFallback) {
        // fallback solver (symmetric SELL-64, 32-bit indices): u and u' in LDS when they fit, everything in HBM otherwise
        HIPCHK(c, WS.vMu.ensure(sizeof(double) * R1)); HIPCHK(c, WS.vCu.ensure(sizeof(double) * R1));
        HIPCHK(c, WS.vMun.ensure(sizeof(double) * R1)); HIPCHK(c, WS.vCun.ensure(sizeof(double) * R1));
        HIPCHK(c, WS.gU.ensure(sizeof(double) * R1)); HIPCHK(c, WS.gUn.ensure(sizeof(double) * R1));
        // Few (large) problems: all compute units solve them together, one after the other (k_solve_wide, cooperative
        // launch so that every workgroup is resident); many: one workgroup per problem, u and u' in LDS when they fit.
        bool coop = D.wide != 0 && c->coop_ok;                  // decided when the batch was scored (enqueue_score / roman_set_matrix_data)
        if (coop) {
            const int G = c->num_cu;
            // Several fallback problems: TEAMS — the workgroups of an XCD (or of half an XCD) solve one problem each, with a
            // one-level barrier among themselves; the whole device on one problem at a time otherwise (one huge problem, or
            // live sets beyond a team's registers: a thread owns WIDE_KW elements).
            int a_teams = 0;
            // The kernel forms its teams from a census of the XCD every workgroup really runs on; the HOST sizes a team's share of
            // the buffers from the XCD count the runtime reports (8 on an MI355X in SPX mode; a CPX partition has 1).  Should the
            // two ever disagree — a team larger than its share of the partials, or too small for a live set — the kernel leaves
            // the problem its pre-written ROMAN_ST_INTERNAL record, and the host-pointer entry points run those problems again
            // with the whole device per problem (roman_ctx_set_wide_teams(ctx, 0) does the same for a device-pointer caller).
            const int perXcd = std::max(1, (G + c->num_xcc - 1) / c->num_xcc);
            {
                constexpr int margin = 2;
                auto cap = [&](int sub) { return (int64_t)WIDE_KW * std::max(1, perXcd / sub - margin) * WIDE_NW * 64; };   // (a margin of two workgroups against uneven placement)
                // more, smaller teams while there are problems for them and the live sets fit their registers: a pass of a team is a stream the
                // whole device's bandwidth bounds however it is shared out, plus two barriers and a collect whose latencies only other teams can
                // hide (64 problems of L = 4 900: 24.7 / 16.9 / 12.4 / 12.1 ms with 1 / 2 / 3 / 4 teams per XCD)
                if (mayFallback >= 2 && maxA <= cap(1)) {
                    a_teams = 1;
                    for (int s_ = 2; s_ <= 4; ++s_) if (mayFallback > 6 * s_ && maxA <= cap(s_)) a_teams = s_;
                    // three teams per XCD WITHOUT the reserve when that is what the live sets need (L = 10 000 = 100 x 100 objects on teams of
                    // 10-11 units): a cooperative launch of one workgroup per unit fills every XCD evenly on this part; should a team come out
                    // smaller after all, its problems keep their ROMAN_ST_INTERNAL records and run again on the whole device (align_chunked)
                    if (a_teams == 2 && mayFallback > 18 && G == c->num_cu && maxA <= (int64_t)WIDE_KW * (perXcd / 3) * WIDE_NW * 64) a_teams = 3;
                }
                // sw.wide_teams (experiments / tests; before roman_ctx_set_wide_teams): 0 never, 1 / 2 / 4 teams per XCD whenever the live sets fit
                const int forced = sw.wide_teams_set ? sw.wide_teams : c->wide_teams;
                if (sw.wide_teams_set || c->wide_teams >= 0) a_teams = (forced >= 1 && forced <= 4 && mayFallback >= 1 && maxA <= cap(forced)) ? forced : 0;
            }
            if (a_teams) c->teams_launched = true;
            const int nTeams = a_teams ? 8 * a_teams : 1;       // (teams are numbered XCC_ID * teams-per-XCD + sub-team: 8 XCC ids whatever the partition)
            const int NWGt = a_teams ? std::min(G, 2 * ((perXcd + a_teams - 1) / a_teams) + 8) * WIDE_NW : G * WIDE_NW;     // waves a team can have at most
            // Pull + push passes over a half copy of the matrix — every pair stored once, rows in a per-block order — (kernels.hip.h, build_upper;
            // an instantiation of its own, k_solve_wide<uint16_t, true>): taken where it was measured faster than the plain kernel — TEAMS on live
            // sets of at least 8 000 associations (break-even ~7 700: L = 7 225 19.1 -> 19.9, L = 8 100 25.8 -> 24.9, L = 9 025 30.0 -> 27.7; 64 x L = 10 000: 39.7 -> 36.6 ms of solve, 96 x: 55.8 -> 52.6, 24 x: 15.9 -> 14.4; L = 8 100:
            // 26.6 -> 25.8) —, not below (L = 4 900: 10.0 -> 12.2, L = 6 400: 27.5 -> 31.3: its passes outside the copy cost more registers and a
            // longer collect) and not with the whole device on one problem (n = m = 200: 22.8 -> 22.4).  sw.wide_upper forces either.
            int a_ucfg = (D.idx16 && a_teams > 0 && maxA >= 8000) ? 1 : 0;
            if (sw.wide_upper != CHOICE_LIB) a_ucfg = (D.idx16 && sw.wide_upper == 1) ? 1 : 0;
            long long a_partStride = (long long)(((size_t)NWGt * WIDE_MAXCH + (size_t)(a_ucfg ? WIDE_MAXBLK : 1) * ((size_t)(maxA + 63) / 64) + 4) * 64 * 2);   // pieces: chunks + slices (per column block of the half copy)
            HIPCHK(c, WS.widePart.ensure(sizeof(double) * (size_t)a_partStride * (size_t)nTeams));
            HIPCHK(c, WS.wideSlots.ensure(sizeof(double) * 2 * (size_t)G * WIDE_NRED * (size_t)nTeams));
            DevParams Dv = D; int Bv = B;
            const ProbDesc* a_probs = WS.probs.as<ProbDesc>(); ProbState* a_state = WS.state.as<ProbState>();
            const double* a_feats = feats; const int32_t* a_assoc = assoc;
            const int32_t* a_lp = WS.lp.as<int32_t>(); const double* a_ld = WS.ld.as<double>();
            const uint32_t* a_perm = WS.perm.as<uint32_t>(); const uint32_t* a_rpos = WS.rowPos.as<uint32_t>(); const uint32_t* a_sb = WS.sliceBase.as<uint32_t>();
            const void* a_cols = D.idx16 ? (const void*)WS.cols16.as<uint16_t>() : (const void*)WS.cols32.as<uint32_t>(); const double* a_vals = WS.vals.as<double>();
            double* a_vU = WS.gU.as<double>(); double* a_vX = WS.gUn.as<double>(); double* a_vX2 = WS.vCun.as<double>();
            double* a_s0 = WS.vMu.as<double>(); double* a_s1 = WS.vCu.as<double>(); double* a_s2 = WS.vMun.as<double>();
            int32_t* a_plp = WS.plp.as<int32_t>();
            const double* a_u0 = u0; SolveOut a_O = O;
            double* a_part = WS.widePart.as<double>(); double* a_slots = WS.wideSlots.as<double>(); unsigned* a_bar = WS.wideBar.as<unsigned>();
            // dynamic LDS: the support bit map of the gathered vector + its leading part (everything the static part leaves of the 160 KB)
            int a_bmw = (int)((maxA + 63) / 64) + 1;
            HIPCHK(c, WS.wideBm.ensure(sizeof(unsigned long long) * 3 * (size_t)a_bmw * (size_t)nTeams));      // two bit maps + the new slice widths of a compaction
            unsigned long long* a_bm = WS.wideBm.as<unsigned long long>();
            // LDS: three bit maps (the multiplied vector's support, the compacted copy's columns, the window's union), the
            // cumulative slice widths of the stream in use, the multiplied vector's leading part
            const int64_t wideFixed = (int64_t)wide_fixed_lds(a_bmw);
            int a_xcap = (int)(((int64_t)c->lds_max - 4096 - wideFixed) / (int64_t)sizeof(double)) & ~63;
            if (a_xcap < 0) a_xcap = 0;
            const size_t wideLds = sizeof(double) * (size_t)a_xcap + (size_t)wideFixed;
            // Column compaction (kernels.hip.h, k_solve_wide): a mirror of the matrix pools holds the compacted copy.
            // sw.wide_compact = 0 turns it off; = 0xWWTTCC sets passes per window / threshold (x/256) / compactions allowed per problem.
            int a_ccfg = 6 | (128 << 8) | (4 << 16);
            if (sw.wide_compact_set) a_ccfg = sw.wide_compact;
            // the pushed sums of the half copy's column blocks (one slot per workgroup of a team) and its slice widths
            int a_ySlots = NWGt / WIDE_NW;
            int a_ycap = a_ucfg ? ((a_xcap / 3) & ~63) : 0;
            if (a_ucfg && a_ycap < 64) a_ucfg = 0;
            if (a_ucfg) {
                HIPCHK(c, WS.wideY.ensure(sizeof(unsigned long long) * 2 * (size_t)a_ycap * (size_t)a_ySlots * (size_t)nTeams));
                HIPCHK(c, WS.wideUp.ensure(sizeof(uint32_t) * 1800 * (size_t)a_bmw * (size_t)nTeams));      // (kernels.hip.h, build_upper: widths, per-block counts / ranks / rows, piece records)
            }
            unsigned long long* a_yPart = WS.wideY.as<unsigned long long>(); uint32_t* a_upMeta = WS.wideUp.as<uint32_t>();
            if ((a_ccfg & 0xff) || a_ucfg) {
                HIPCHK(c, WS.valsC.ensure(sizeof(double) * (size_t)WS.capNnz));
                HIPCHK(c, WS.colsC.ensure((D.idx16 ? sizeof(uint16_t) : sizeof(uint32_t)) * (size_t)WS.capNnz));
            }
            void* a_colsC = WS.colsC.p; double* a_valsC = WS.valsC.as<double>();
            const void* wideFn = D.idx16 ? (a_ucfg ? reinterpret_cast<const void*>(k_solve_wide<uint16_t, true>) : reinterpret_cast<const void*>(k_solve_wide<uint16_t, false>))
                                         : reinterpret_cast<const void*>(k_solve_wide<uint32_t, false>);
            HIPCHK(c, dyn_lds(c, wideFn, wideLds));
            unsigned long long a_ticks = c->spin_ticks;        // 4 s of the device's wall clock (test hook ROMAN_WIDE_SPIN_MS: shorter)
            const int32_t* a_fb = WS.fbList.as<int32_t>();
            void* args[] = {&Dv, &Bv, &a_probs, &a_state, &a_feats, &a_assoc, &a_lp, &a_ld, &a_perm, &a_rpos, &a_sb, &a_cols, &a_vals,
                            &a_vU, &a_vX, &a_vX2, &a_s0, &a_s1, &a_s2, &a_plp, &a_u0, &a_O, &a_part, &a_slots, &a_bar, &a_bm, &a_bmw, &a_xcap, &a_ticks,
                            &a_teams, &a_fb, &a_partStride, &a_colsC, &a_valsC, &a_ccfg, &a_ucfg, &a_yPart, &a_ySlots, &a_ycap, &a_upMeta};
            // Two whole-device kernels must never be resident together (each would hold compute units while waiting at a
            // grid barrier for workgroups the other one keeps out): with batches in flight on several streams, a
            // launch waits for the previous one of this context.
            if (!c->coopDone) HIPCHK(c, hipEventCreateWithFlags(&c->coopDone, hipEventDisableTiming));
            if (c->coopIssued) HIPCHK(c, hipStreamWaitEvent(WS.stream, c->coopDone, 0));
            const hipError_t e = hipLaunchCooperativeKernel(wideFn, dim3((unsigned)G), dim3(WIDE_NT), args, wideLds, WS.stream);
            if (e == hipSuccess) { HIPCHK(c, hipEventRecord(c->coopDone, WS.stream)); c->coopIssued = true; }
            if (e != hipSuccess) {                              // not available here: the one-workgroup solver does the same work
                (void)hipGetLastError();
                fprintf(stderr, "[roman_hip] cooperative launch failed (%s); large problems use the single-workgroup solver\n", hipGetErrorString(e));
                c->coop_ok = false; coop = false;
                if (D.idx16) return fail(c, ROMAN_E_HIP, "cooperative launch of the large-problem solver failed (%s); run the call again (it now takes the single-workgroup solver)", hipGetErrorString(e));
            }
    DBG(c, "k_solve_wide");
        }
        if (!coop) {
        const size_t fixed = 72 * sizeof(double) + 4 * sizeof(int);
        const int Lcap = (int)(((c->lds_max - fixed) / (2 * sizeof(double))) & ~(size_t)1);
        const size_t lds = (size_t)2 * sizeof(double) * (size_t)Lcap + fixed;
        const int grid = std::max(1, std::min(B, c->num_cu));
        HIPCHK(c, dyn_lds(c, reinterpret_cast<const void*>(k_solve<uint32_t, 1>), lds));
        hipLaunchKernelGGL((k_solve<uint32_t, 1>), dim3(grid), dim3(1024), lds, WS.stream, D, B, WS.probs.as<ProbDesc>(), WS.state.as<ProbState>(), feats, assoc,
                           WS.lp.as<int32_t>(), WS.ld.as<double>(), WS.perm.as<uint32_t>(), WS.rowPos.as<uint32_t>(), WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.cols32.as<uint32_t>(), WS.vals.as<double>(),
                           WS.vMu.as<double>(), WS.vCu.as<double>(), WS.vMun.as<double>(), WS.vCun.as<double>(), WS.gU.as<double>(), WS.gUn.as<double>(),
                           WS.plp.as<int32_t>(), WS.pld.as<double>(), u0, O, WS.queue.as<int>() + 4, Lcap);
        }
    DBG(c, "k_solve");
    }
    t3.stop();
    HIPCHK(c, hipGetLastError());
#ifdef ROMAN_SOLVE_TIMING
    {
        std::vector<unsigned long long> h((size_t)B * 16);
        HIPCHK(c, hipMemcpyAsync(h.data(), WS.hAux3.p, sizeof(unsigned long long) * 16 * (size_t)B, hipMemcpyDeviceToHost, WS.stream));
        HIPCHK(c, hipStreamSynchronize(WS.stream));
        double acc[16] = {0};
        for (int b = 0; b < B; ++b) for (int t = 0; t < 16; ++t) acc[t] += (double)h[(size_t)b * 16 + t];
        // (k_solve_up: cycles of the phases named here; k_solve_wide: 10 ns ticks of trial+publish, barrier 1, stream, barrier 2,
        //  collect+objective, barrier 3, everything else — in slots 0..6)
        const char* nm[8] = {"stream", "spmv-barrier", "decode", "elementwise", "stream-narrow", "setup+tail", "publish", "red-sums"};
        fprintf(stderr, "[solve timing] B=%d cycles/problem:", B);
        double tot_ = 0; for (int t = 0; t < 8; ++t) tot_ += acc[t] / B;
        for (int t = 0; t < 8; ++t) fprintf(stderr, " %s %.0f (n=%.1f)", nm[t], acc[t] / B, acc[8 + t] / B);
        fprintf(stderr, " total %.0f\n", tot_);
        if (B > 1) {   // the slowest problems
            std::vector<std::pair<double, int>> tt;
            for (int b = 0; b < B; ++b) { double t_ = 0; for (int t = 0; t < 8; ++t) t_ += (double)h[(size_t)b * 16 + t]; tt.push_back({t_, b}); }
            std::sort(tt.begin(), tt.end());
            for (int r = 0; r < 3; ++r) {
                const int b = tt[(size_t)(B - 1 - r)].second;
                fprintf(stderr, "   slow #%d (b=%d, %.0f cyc):", r, b, tt[(size_t)(B - 1 - r)].first);
                for (int t = 0; t < 8; ++t) fprintf(stderr, " %s %.0f (n=%.0f)", nm[t], (double)h[(size_t)b * 16 + t], (double)h[(size_t)b * 16 + 8 + t]);
                fprintf(stderr, "\n");
            }
            fprintf(stderr, "   median problem: %.0f cyc\n", tt[(size_t)B / 2].first);
        }
    }
#endif
    return ROMAN_OK;
}

// how many problems of the batch can be of the fallback kind (0: none, the fallback solver is not launched)
int may_fallback(const DevParams& D, const std::vector<ProbDesc>& hd)
{
    if (!D.allow_fallback) return 0;
    if (D.p.maxiniters < 1 || D.p.maxlsiters < 1) return (int)hd.size();
    int n = 0;
    for (const ProbDesc& d : hd) if (d.nA > D.stream_maxL) ++n;
    return n;
}

int ensure_events(roman_ctx* c)
{
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k)
        for (int s = 0; s < ROMAN_STAGE_COUNT; ++s) {
            if (!c->ws[k].evA[s]) HIPCHK(c, hipEventCreate(&c->ws[k].evA[s]));
            if (!c->ws[k].evB[s]) HIPCHK(c, hipEventCreate(&c->ws[k].evB[s]));
        }
    return ROMAN_OK;
}

// one batch through the stages, on workspace c->cur and its stream (pure enqueue)
int run_batch(roman_ctx* c, const DevParams& D0, const roman_params_t* params, const BatchIn& in, const double* u0, const BatchOut& out)
{
    std::vector<ProbDesc> hd;
    DevParams D;
    int rc = enqueue_score(c, D0, params, in, hd, &D, &out, u0);
    if (rc) return rc;
    int64_t sumA = 0, maxA = 0; for (const ProbDesc& d : hd) { sumA += d.nA; maxA = std::max<int64_t>(maxA, d.nA); }
    return enqueue_solve(c, D, in.B, sumA, maxA, in.feats, in.assoc, u0, false, may_fallback(D, hd), out);
}

// After a synchronous run: did every problem fit its workspace?  (reads the totals the batch copied back; the stream
// has been synchronised by the caller).  On overflow the history now holds the need: the caller runs the batch again.
bool batch_overflowed(roman_ctx* c)
{
    harvest_totals(c, true);
    const BatchTotals& t = *WS.pinnedTotals;
    if (switches_once().debug) fprintf(stderr, "[roman] batch totals: R=%d maxL=%d items=%d maskWords need %lld cap %lld, nnz need %lld cap %lld, list need %llu cap %lld, overflow=%d sliceGroups=%d\n",
                     t.R, t.maxL, t.items, (long long)t.needMaskWords, WS.capMaskWords, (long long)t.needNnz, WS.capNnz, t.listTop, WS.capList, t.overflow, t.sliceGroups);
    return t.overflow > 0;
}

// run a B=1 solve on the matrices held by the context and pull the solution to the host
int solve_last(roman_ctx* c, const double* u0_host)
{
    roman_ctx::Last& Lst = c->last;
    const int32_t nA = Lst.nA;
    const size_t nA1 = (size_t)std::max(nA, 1);
    const double* dU0 = nullptr;
    if (u0_host) {
        HIPCHK(c, WS.hU0.ensure(sizeof(double) * nA1));
        HIPCHK(c, hipMemcpyAsync(WS.hU0.p, u0_host, sizeof(double) * (size_t)nA, hipMemcpyHostToDevice, WS.stream));
        dU0 = WS.hU0.as<double>();
    }
    const int32_t kmax = std::max(nA, 1);
    HIPCHK(c, WS.oAssoc.ensure(sizeof(int32_t) * 2 * (size_t)kmax)); HIPCHK(c, WS.oN.ensure(sizeof(int32_t)));
    HIPCHK(c, WS.oT.ensure(sizeof(double) * 16)); HIPCHK(c, WS.oStatus.ensure(sizeof(int32_t))); HIPCHK(c, WS.oStats.ensure(sizeof(roman_stats_t)));
    const double* feats = Lst.dense ? nullptr : WS.hFeats.as<double>();
    const int32_t* assoc = (Lst.pd.assocOff >= 0) ? WS.hAssoc.as<int32_t>() : nullptr;
    const BatchOut out{kmax, WS.oAssoc.as<int32_t>(), WS.oN.as<int32_t>(), WS.oT.as<double>(), WS.oStatus.as<int32_t>(), WS.oStats.as<roman_stats_t>()};
    int rc = enqueue_solve(c, Lst.D, 1, nA, nA, feats, assoc, dU0, Lst.hascz, Lst.kind == 1 ? 1 : 0, out);
    if (rc) return rc;
    int32_t nsel = 0;
    HIPCHK(c, hipMemcpyAsync(&nsel, WS.nSel.p, sizeof(int32_t), hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipMemcpyAsync(&Lst.stats, WS.oStats.p, sizeof(roman_stats_t), hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipMemcpyAsync(&Lst.status, WS.oStatus.p, sizeof(int32_t), hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    if (Lst.status & ROMAN_ST_INTERNAL) return fail(c, ROMAN_E_INTERNAL, "the solve reported ROMAN_ST_INTERNAL: a bounded wait of the whole-device solver expired");
    Lst.nsel = nsel;
    Lst.nodes.assign((size_t)std::max(nsel, 0), 0);
    const int L = Lst.L;
    std::vector<double> ul((size_t)std::max(L, 1)); std::vector<int32_t> lpv((size_t)std::max(L, 1));
    if (nsel > 0) HIPCHK(c, hipMemcpyAsync(Lst.nodes.data(), WS.nodesOrig.p, sizeof(int32_t) * (size_t)nsel, hipMemcpyDeviceToHost, WS.stream));
    if (L > 0) {
        // u comes back indexed like the solver's vectors: by position (stream layout) or by live index (fallback);
        // the matching association-index pool maps either to the caller's association order
        HIPCHK(c, hipMemcpyAsync(ul.data(), WS.uOut.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, WS.stream));
        HIPCHK(c, hipMemcpyAsync(lpv.data(), Lst.kind == 0 ? WS.plp.p : WS.lp.p, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, WS.stream));
    }
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    Lst.u.assign((size_t)nA, 0.0);
    for (int k = 0; k < L; ++k) Lst.u[(size_t)lpv[k]] = ul[k];
    Lst.solved = true;
    return ROMAN_OK;
}

// Download the matrix of the last single problem and decode it into per-row lists over LIVE indices, both triangles,
// ascending columns: rs/rl index into cols/vals (row-contiguous on return; bit 31 of a column = "C_pq == 0"); inert
// slots are dropped.  lp / diag: association index and diagonal value per live index.
int fetch_last_csr(const roman_ctx* cc, std::vector<uint32_t>& rs, std::vector<uint32_t>& rl, std::vector<uint32_t>& cols,
                   std::vector<double>& vals, std::vector<int32_t>& lp, std::vector<double>& ls)
{
    roman_ctx* c = const_cast<roman_ctx*>(cc);
    const roman_ctx::Last& Lst = c->last;
    const int L = Lst.L; const int64_t cap = Lst.nnzCap;
    const size_t L1 = (size_t)std::max(L, 1), cap1 = (size_t)std::max<int64_t>(cap, 1);
    std::vector<uint32_t> jcnt(L1, 0), jpos(L1, 0), jperm(L1, 0), jsw(L1, 0), jsb(L1, 0), jcols(cap1, 0); std::vector<double> jvals(cap1, 0.0);
    rs.assign(L1, 0); rl.assign(L1, 0); lp.assign(L1, 0); ls.assign(L1, 0.0);
    HIPCHK(c, hipSetDevice(c->device));
    roman_ctx::Workspace& W0 = c->ws[0];
    const bool up = Lst.kind == 0;
    if (L > 0) {
        const int nsl = (L + 63) / 64;
        HIPCHK(c, hipMemcpy(jcnt.data(), W0.rowCnt.p, sizeof(uint32_t) * (size_t)L, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(jpos.data(), W0.rowPos.p, sizeof(uint32_t) * (size_t)L, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(jperm.data(), W0.perm.p, sizeof(uint32_t) * (size_t)L, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(jsw.data(), W0.sliceWidth.p, sizeof(uint32_t) * (size_t)nsl, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(jsb.data(), W0.sliceBase.p, sizeof(uint32_t) * (size_t)nsl, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(lp.data(), W0.lp.p, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ls.data(), W0.ld.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost));   // diagonal values
    }
    if (cap > 0) {
        HIPCHK(c, hipMemcpy(jvals.data(), W0.vals.p, sizeof(double) * (size_t)cap, hipMemcpyDeviceToHost));
        if (up) {
            std::vector<uint16_t> c16((size_t)cap);
            HIPCHK(c, hipMemcpy(c16.data(), W0.cols16.p, sizeof(uint16_t) * (size_t)cap, hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < cap; ++k) jcols[(size_t)k] = (c16[(size_t)k] & 0x8000u) ? (0x80000000u | (c16[(size_t)k] & 0x7fffu)) : c16[(size_t)k];
        } else if (Lst.D.idx16) {                               // fallback layout with 16-bit labels: 0xffff = inert
            std::vector<uint16_t> c16((size_t)cap);
            HIPCHK(c, hipMemcpy(c16.data(), W0.cols16.p, sizeof(uint16_t) * (size_t)cap, hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < cap; ++k) jcols[(size_t)k] = (c16[(size_t)k] == 0xffffu) ? 0xffffffffu : (uint32_t)c16[(size_t)k];
        } else {
            HIPCHK(c, hipMemcpy(jcols.data(), W0.cols32.p, sizeof(uint32_t) * (size_t)cap, hipMemcpyDeviceToHost));
        }
    }
    std::vector<std::vector<std::pair<uint32_t, double>>> rows(L1);
    if (up) {
        // stream layout: row p (POSITION) holds its strict-upper entries (p, q), q a position; rowCnt[p] slots are in use
        for (int p = 0; p < L; ++p) {
            const uint32_t sl = (uint32_t)p >> 6, slot = (uint32_t)p & 63u;
            const uint32_t kp = jperm[(size_t)p];
            for (uint32_t e = 0; e < ((jcnt[(size_t)p] + 3u) & ~3u); ++e) {                         // (every slot of the row's quads: the fill may rotate them)
                const uint32_t cq = jcols[h_col_pos(true, jsb[sl], slot, e)]; const double v = jvals[h_val_pos(true, jsb[sl], slot, e)];
                const uint32_t q = cq & 0x7fffffffu;
                if (q >= (uint32_t)L) continue;                                                      // inert slot (dummy column L + slot)
                const uint32_t kq = jperm[(size_t)q], flag = cq & 0x80000000u;
                rows[kp].push_back({kq | flag, v}); rows[kq].push_back({kp | flag, v});
            }
        }
    } else {
        for (int k = 0; k < L; ++k) {
            const uint32_t pos = jpos[(size_t)k], sl = pos >> 6, slot = pos & 63u;
            for (uint32_t e = 0; e < jcnt[(size_t)k]; ++e) {
                const uint32_t cq = jcols[h_col_pos(true, jsb[sl], slot, e)]; const double v = jvals[h_val_pos(true, jsb[sl], slot, e)];
                if (cq == 0xffffffffu || (v == 0.0 && (cq & 0x80000000u) && (cq & 0x7fffffffu) == pos)) continue;   // inert slot (16-bit: no column; 32-bit: the row's own position, flagged)
                rows[(size_t)k].push_back({jperm[(size_t)(cq & 0x7fffffffu)] | (cq & 0x80000000u), v});     // column labels are positions
            }
        }
    }
    cols.clear(); vals.clear();
    for (int k = 0; k < L; ++k) {
        auto& r = rows[(size_t)k];
        std::sort(r.begin(), r.end(), [](const std::pair<uint32_t, double>& a, const std::pair<uint32_t, double>& b) { return (a.first & 0x7fffffffu) < (b.first & 0x7fffffffu); });
        rs[(size_t)k] = (uint32_t)cols.size();
        for (auto& e : r) { cols.push_back(e.first); vals.push_back(e.second); }
        rl[(size_t)k] = (uint32_t)r.size();
    }
    if (cols.empty()) { cols.push_back(0); vals.push_back(0.0); }
    return ROMAN_OK;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* roman_version(void) { return "roman_hip 0.2.0 gfx950 (HIP, wave64, f64)"; }

int roman_params_default(roman_params_t* p)
{
    if (!p) return fail(nullptr, ROMAN_E_INVALID, "params is NULL");
    memset(p, 0, sizeof(*p));
    p->invariant = ROMAN_INV_ROMAN; p->point_dim = 3; p->fusion_method = ROMAN_FUSE_GEOMETRIC_MEAN; p->rescale_u0 = 1;
    p->sigma = 0.4; p->epsilon = 0.6; p->mindist = 0.2;
    p->distance_weight = p->ratio_weight = p->cosine_weight = 1.0;
    p->cosine_min = 0.5; p->cosine_max = 0.7; p->gravity_unc_ang_rad = 0.0872665;
    p->tol_u = 1e-8; p->tol_F = 1e-9; p->beta = 0.25; p->eps = 1e-9; p->affinityeps = 1e-4;
    p->maxiniters = 200; p->maxoliters = 1000; p->maxlsiters = 99;
    return ROMAN_OK;
}

const char* roman_last_error(const roman_ctx_t* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int roman_ctx_create(roman_ctx_t** out, int device, void* stream)
{
    if (!out) return fail(nullptr, ROMAN_E_INVALID, "ctx out pointer is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(nullptr, ROMAN_E_NO_DEVICE, "no HIP device visible (libroman_hip has no CPU fallback)"); }
    if (device < 0 || device >= ndev) return fail(nullptr, ROMAN_E_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, ROMAN_E_HIP, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, ROMAN_E_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(nullptr, ROMAN_E_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    roman_ctx* c = new (std::nothrow) roman_ctx();
    if (!c) return fail(nullptr, ROMAN_E_NOMEM, "out of host memory");
    c->device = device;
    const Switches sw = read_switches();
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {   // XCDs of this device (8 on an MI355X in SPX mode, 1 in CPX mode): the team mode of k_solve_wide sizes a team's buffers from it
        int nx = 0;
        if (hipDeviceGetAttribute(&nx, hipDeviceAttributeNumberOfXccs, device) != hipSuccess || nx < 1 || nx > 8) { (void)hipGetLastError(); nx = 8; }
        if (sw.num_xcc) nx = sw.num_xcc;                           // test hook: a host-side count that does not match the device's
        c->num_xcc = nx;
    }
    c->lds_max = prop.sharedMemPerBlock >= 163840 ? (size_t)(160 * 1024 - 256) : (size_t)prop.sharedMemPerBlock;
    { int coopAttr = 0; c->coop_ok = hipDeviceGetAttribute(&coopAttr, hipDeviceAttributeCooperativeLaunch, device) == hipSuccess && coopAttr != 0; (void)hipGetLastError(); }
    if (c->coop_ok) {
        // The whole-device solver is chosen when a batch is SCORED (16-bit labels are written for it): make sure here, once,
        // that one 512-thread workgroup with its largest dynamic LDS fits a compute unit for both instantiations — a
        // cooperative launch of num_cu workgroups then cannot fail for lack of residency after the fill has already run.
        const size_t wideLdsMax = c->lds_max > 4096 ? c->lds_max - 4096 : 0;
        const void* fns[3] = {reinterpret_cast<const void*>(k_solve_wide<uint16_t, false>), reinterpret_cast<const void*>(k_solve_wide<uint32_t, false>),
                              reinterpret_cast<const void*>(k_solve_wide<uint16_t, true>)};
        for (const void* fn : fns) {
            int nb = 0;
            if (dyn_lds(c, fn, wideLdsMax) != hipSuccess ||
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, WIDE_NT, wideLdsMax) != hipSuccess || nb < 1) { (void)hipGetLastError(); c->coop_ok = false; }
        }
    }
    {   // wall_clock64() ticks at the rate the runtime reports (kHz; 100 MHz on this part)
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) { (void)hipGetLastError(); khz = 100000; }
        double ms = 4000.0;
        if (sw.wide_spin_ms >= 0.0) ms = sw.wide_spin_ms;          // test hook (0: the first unsuccessful poll of a wait is a timeout)
        c->spin_ticks = (unsigned long long)((double)khz * ms);
    }
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(nullptr, ROMAN_E_HIP, "hipStreamCreate failed"); }
        c->own_stream = true;
    }
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) c->ws[k].stream = c->stream;
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) {
        if (hipHostMalloc((void**)&c->ws[k].pinnedTotals, sizeof(BatchTotals), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&c->ws[k].totEvent, hipEventDisableTiming) != hipSuccess) {
            roman_ctx_destroy(c); return fail(nullptr, ROMAN_E_NOMEM, "hipHostMalloc / hipEventCreate failed");
        }
        memset(c->ws[k].pinnedTotals, 0, sizeof(BatchTotals));
    }
    *out = c;
    return ROMAN_OK;
}

int roman_ctx_destroy(roman_ctx_t* c)
{
    if (!c) return ROMAN_OK;
    (void)hipSetDevice(c->device);
    (void)roman_ctx_sync(c);
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) {
        roman_ctx::Workspace& W = c->ws[k];
        DevBuf* all[] = {&W.probs, &W.state, &W.totals, &W.queue, &W.cosPool, &W.cosDense, &W.tabPool, &W.qtabPool, &W.sTmp, &W.chunkCnt,
                         &W.lp, &W.li, &W.lj, &W.ls, &W.ld, &W.lza, &W.lzb, &W.plp, &W.pli, &W.plj, &W.pls, &W.pld, &W.plza, &W.plzb,
                         &W.rowCnt, &W.rowPos, &W.perm, &W.sliceWidth, &W.sliceBase, &W.items, &W.maskPool, &W.prefPool, &W.listPool, &W.listOff,
                         &W.vMu, &W.vCu, &W.vMun, &W.vCun, &W.gU, &W.gUn, &W.uOut, &W.nodesOrig, &W.nSel, &W.widePart, &W.wideSlots, &W.wideBar, &W.wideBm, &W.wideY, &W.wideUp, &W.fbList, &W.cols16, &W.cols32, &W.vals, &W.colsC, &W.valsC,
                         &W.hFeats, &W.hAssoc, &W.hU0, &W.oAssoc, &W.oN, &W.oT, &W.oStatus, &W.oStats, &W.hAux1, &W.hAux2, &W.hAux3, &W.oAll, &W.lcStage, &W.mnoVals, &W.mnoOut, &W.mnoHost};
        for (DevBuf* b : all) b->release();
        if (W.pinnedTotals) (void)hipHostFree(W.pinnedTotals);
        if (W.totEvent) (void)hipEventDestroy(W.totEvent);
        W.probStage.release();
        for (int s = 0; s < ROMAN_STAGE_COUNT; ++s) { if (W.evA[s]) (void)hipEventDestroy(W.evA[s]); if (W.evB[s]) (void)hipEventDestroy(W.evB[s]); }
        if (W.done) (void)hipEventDestroy(W.done);
    }
    if (c->hostOut) (void)hipHostFree(c->hostOut);
    { DevBuf* share[] = {&c->shareDesc, &c->shareIds, &c->shareKeep, &c->shareKept, &c->shareJobs}; for (DevBuf* b : share) b->release(); }
    c->hostMirror.release(); c->ransacDesc.release();
    c->shareStage.release(); c->ransacStage.release();
    { DevBuf* sm[] = {&c->smJobs, &c->smPts, &c->smSpillKey, &c->smSpillIdx, &c->smListOut}; for (DevBuf* b : sm) b->release(); }
    c->smStage.release();
    c->ggNorm.release(); c->sgCount.release();
    c->ssNorm.release(); c->ssBand.release(); c->ssR.release(); c->ssItems.release(); c->ssStage.release();
    c->sfTab.release(); c->sfStage.release();
    c->segItems.release(); c->segStage.release();
    c->asKeys.release(); c->asScratch.release(); c->asRec.release(); c->asNorm.release(); c->asItems.release(); c->asStage.release();
    c->sgPts.release(); c->sgDs.release(); c->sgKeys.release(); c->sgKeys2.release(); c->sgIdx.release(); c->sgIdx2.release();
    c->sgAvg.release(); c->sgM.release(); c->sgItems.release(); c->sgStage.release();
    c->clPar.release(); c->clAux.release(); c->clHist.release(); c->clLab.release(); c->clItems.release(); c->clStage.release();
    if (c->evIn) (void)hipEventDestroy(c->evIn);
    if (c->coopDone) (void)hipEventDestroy(c->coopDone);
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) if (c->istream[k]) (void)hipStreamDestroy(c->istream[k]);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return ROMAN_OK;
}

// Batches in flight.  depth 1 (default): every call runs on the context's stream.  depth 2 or 3: batch calls
// (roman_align_batch_dev) rotate over that many workspaces, each with an internal stream that starts after
// the work already queued on the context's stream; their results are complete after roman_ctx_sync (or a
// device-wide synchronisation), NOT after synchronising the context's stream alone.
int roman_ctx_set_pipeline(roman_ctx_t* c, int depth)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (depth < 1 || depth > ROMAN_MAX_PIPELINE) return fail(c, ROMAN_E_INVALID, "pipeline depth must be 1..%d", ROMAN_MAX_PIPELINE);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = roman_ctx_sync(c);
    if (rc) return rc;
    if (depth >= 2) {
        for (int k = 0; k < depth; ++k) {
            if (!c->istream[k]) HIPCHK(c, hipStreamCreateWithFlags(&c->istream[k], hipStreamNonBlocking));
            if (!c->ws[k].done) HIPCHK(c, hipEventCreateWithFlags(&c->ws[k].done, hipEventDisableTiming));
        }
        if (!c->evIn) HIPCHK(c, hipEventCreateWithFlags(&c->evIn, hipEventDisableTiming));
    }
    c->pipeline = depth; c->next_ws = 0; c->cur = 0; c->latest_ws = -1;
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) { c->ws[k].issued = false; c->ws[k].stream = c->stream; }
    return ROMAN_OK;
}

// Make the context's (caller's) stream wait — without blocking the host — for the pipelined batches issued so
// far: all of them (skip_latest == 0) or all but the most recent one (skip_latest != 0), so that work queued on
// the caller's stream afterwards (e.g. the RCCL all_gather of batch k-1's records) sees their results while the
// latest batch keeps running.
int roman_ctx_join_on(roman_ctx_t* c, int skip_latest, void* stream)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t target = stream ? (hipStream_t)stream : c->stream;
    if (c->pipeline < 2) {                                      // everything runs on the context's stream: another stream waits for what is queued there
        if (target != c->stream) {
            if (!c->evIn) HIPCHK(c, hipEventCreateWithFlags(&c->evIn, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(c->evIn, c->stream));
            HIPCHK(c, hipStreamWaitEvent(target, c->evIn, 0));
        }
        return ROMAN_OK;
    }
    for (int k = 0; k < c->pipeline; ++k) {
        if (skip_latest && k == c->latest_ws) continue;
        if (c->ws[k].done && c->ws[k].issued) HIPCHK(c, hipStreamWaitEvent(target, c->ws[k].done, 0));
    }
    return ROMAN_OK;
}

int roman_ctx_join(roman_ctx_t* c, int skip_latest) { return roman_ctx_join_on(c, skip_latest, nullptr); }

int roman_ctx_sync(roman_ctx_t* c)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) if (c->istream[k]) HIPCHK(c, hipStreamSynchronize(c->istream[k]));
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    return ROMAN_OK;
}

int roman_ctx_skipped(roman_ctx_t* c, int wait, int64_t* n)
{
    if (!c || !n) return fail(c, ROMAN_E_INVALID, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (wait) { int rc = roman_ctx_sync(c); if (rc) return rc; }
    harvest_totals(c, wait != 0);
    *n = (int64_t)c->skippedTotal;
    return ROMAN_OK;
}

// --- instrumentation -----------------------------------------------------------------------------
int roman_profile_enable(roman_ctx_t* c, int on)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    if (on) { int rc = ensure_events(c); if (rc) return rc; }
    else for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) for (int s = 0; s < ROMAN_STAGE_COUNT; ++s) prof_flush(c, k, s);
    c->profile = on != 0;
    return ROMAN_OK;
}
int roman_profile_reset(roman_ctx_t* c)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) for (int s = 0; s < ROMAN_STAGE_COUNT; ++s) prof_flush(c, k, s);
    for (int s = 0; s < ROMAN_STAGE_COUNT; ++s) { c->prof_ms[s] = 0.0; c->prof_n[s] = 0; }
    return ROMAN_OK;
}
int roman_profile_get(roman_ctx_t* c, double ms[ROMAN_STAGE_COUNT], int64_t launches[ROMAN_STAGE_COUNT])
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    for (int k = 0; k < ROMAN_MAX_PIPELINE; ++k) for (int s = 0; s < ROMAN_STAGE_COUNT; ++s) prof_flush(c, k, s);
    for (int s = 0; s < ROMAN_STAGE_COUNT; ++s) { if (ms) ms[s] = c->prof_ms[s]; if (launches) launches[s] = c->prof_n[s]; }
    return ROMAN_OK;
}

}  // extern "C"

namespace {
// The loop-closure tail of a call: switches, device inputs, device outputs.
struct LcTail { roman_lc_params_t P; LcIn in; roman_lc_record_t* rec; int32_t* idx; int32_t* cnt; };

int check_lc_params(roman_ctx* c, const roman_lc_params_t* lp)
{
    if (!lp) return fail(c, ROMAN_E_INVALID, "lc_params is NULL");
    if (lp->dim != 2 && lp->dim != 3) return fail(c, ROMAN_E_INVALID, "lc_params.dim must be 2 or 3 (got %d)", lp->dim);
    if (lp->reserved[0] != 0 || lp->reserved[1] != 0) return fail(c, ROMAN_E_INVALID, "roman_lc_params_t.reserved must be 0");
    if (lp->tilt_thresh != lp->tilt_thresh) return fail(c, ROMAN_E_INVALID, "lc_params.tilt_thresh is NaN");
    return ROMAN_OK;
}

int make_lc_tail(roman_ctx* c, const roman_lc_params_t* lp, const double* T, const int32_t* n_assoc, const int32_t* status,
                 const double* T_ref, const int32_t* enable, const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                 roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted, LcTail* t)
{
    int rc = check_lc_params(c, lp);
    if (rc) return rc;
    if (!n_accepted) return fail(c, ROMAN_E_INVALID, "n_accepted is NULL");
    if ((FL != nullptr) != (iL != nullptr) || (FR != nullptr) != (iR != nullptr)) return fail(c, ROMAN_E_INVALID, "a frame pool and its index array come together (FL with iL, FR with iR)");
    t->P = *lp;
    t->in = LcIn{T, n_assoc, status, T_ref, enable, FL, iL, FR, iR};
    t->rec = records; t->idx = accepted_idx; t->cnt = n_accepted;
    return ROMAN_OK;
}

// k_lc_tail + k_lc_compact behind whatever is queued on `stream`
int enqueue_lc_tail(roman_ctx* c, hipStream_t stream, int B, const LcTail& t)
{
    if (B > 0) {
        if (!t.in.T || !t.in.n_assoc || !t.in.status || !t.rec || !t.idx) return fail(c, ROMAN_E_INVALID, "NULL pointer in the loop-closure tail's arguments");
        hipLaunchKernelGGL(k_lc_tail, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, t.P, (int)B, t.in, t.rec);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_lc_compact, dim3(1), dim3(B > 256 ? 1024 : 256), 0, stream, (int)B, (const roman_lc_record_t*)t.rec, t.idx, t.cnt);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// --- what the batch entry points share ---------------------------------------------------------------
// What an entry point knows about its batch besides the four metadata arrays (host arrays for every entry point).
struct BatchCheck {
    int64_t n_objects = -1;                    // rows of the pool the offsets index; -1: not known here (device-pointer callers)
    const int32_t* assoc = nullptr; const int64_t* assoc_off = nullptr;
    bool assoc_on_host = false;                // `assoc` can be read here: its indices are range-checked (a device array never is)
    bool whole_list = false;                   // assoc_off starts at 0 (not so for the slices of it the chunked host entry points hand the device-pointer ones)
    int32_t side_cap = 0; int cap_code = ROMAN_OK; const char* cap_who = "";   // the largest map the entry point serves (0: no cap)
};

// The one check of a batch's metadata (B > 0).  Only host-readable metadata is read, and the bulk array `assoc` only where the
// caller says it is a host array.  `any`: some problem has objects (the callers that need a non-NULL pool then).
int check_batch(roman_ctx* c, int32_t B, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, const BatchCheck& k, bool* any = nullptr)
{
    if (!off1 || !n1 || !off2 || !n2) return fail(c, ROMAN_E_INVALID, "NULL metadata pointer");
    if (k.assoc && !k.assoc_off) return fail(c, ROMAN_E_INVALID, "assoc given without assoc_off");
    if (k.assoc && k.whole_list && k.assoc_off[0] != 0) return fail(c, ROMAN_E_INVALID, "assoc_off[0] must be 0");
    bool some = false;
    for (int b = 0; b < B; ++b) {
        if (n1[b] < 0 || n2[b] < 0 || off1[b] < 0 || off2[b] < 0) return fail(c, ROMAN_E_INVALID, "problem %d: negative size or offset", b);
        if (k.side_cap > 0 && (n1[b] > k.side_cap || n2[b] > k.side_cap)) return fail(c, k.cap_code, "problem %d has %d x %d objects; %s serves at most %d per side", b, n1[b], n2[b], k.cap_who, k.side_cap);
        if (k.n_objects >= 0 && (off1[b] + n1[b] > k.n_objects || off2[b] + n2[b] > k.n_objects))
            return fail(c, ROMAN_E_INVALID, "problem %d reads objects outside the pool's rows [0..%lld)", b, (long long)k.n_objects);
        if (k.assoc) {
            if (k.assoc_off[b + 1] < k.assoc_off[b]) return fail(c, ROMAN_E_INVALID, "assoc_off is not non-decreasing at problem %d", b);
            if (k.assoc_on_host)
                for (int64_t r = k.assoc_off[b]; r < k.assoc_off[b + 1]; ++r)
                    if (k.assoc[2 * r] < 0 || k.assoc[2 * r] >= n1[b] || k.assoc[2 * r + 1] < 0 || k.assoc[2 * r + 1] >= n2[b])
                        return fail(c, ROMAN_E_INVALID, "problem %d: association %lld = (%d,%d) out of range", b, (long long)(r - k.assoc_off[b]), k.assoc[2 * r], k.assoc[2 * r + 1]);
        }
        some = some || n1[b] > 0 || n2[b] > 0;
    }
    if (any) *any = some;
    return ROMAN_OK;
}

// One call of a device-pointer entry point: `work(stream)` enqueues it on workspace 0 and the context's stream (depth 1) or, at
// depth >= 2, on the next workspace of the rotation, whose internal stream starts behind the work already queued on the caller's
// stream.  After an error the workspace's `done` is not recorded and it does not count as issued; c->cur is 0 again either way.
template <typename Work> int on_next_workspace(roman_ctx* c, Work work)
{
    int k = 0;
    if (c->pipeline >= 2) {
        k = c->next_ws;
        c->next_ws = (c->next_ws + 1) % c->pipeline; c->latest_ws = k;
        HIPCHK(c, hipEventRecord(c->evIn, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->istream[k], c->evIn, 0));
    }
    c->cur = k; c->ws[k].stream = c->pipeline >= 2 ? c->istream[k] : c->stream;
    int rc = work(c->ws[k].stream);
    if (!rc && c->pipeline >= 2) {
        const hipError_t e = hipEventRecord(c->ws[k].done, c->ws[k].stream);
        if (e == hipSuccess) c->ws[k].issued = true;
        else { (void)hipGetLastError(); rc = fail(c, ROMAN_E_HIP, "hipEventRecord failed: %s", hipGetErrorString(e)); }
    }
    c->cur = 0; c->last.scored = false; c->last.solved = false;   // workspace 0 is reused: the stepwise problem it held is gone
    return rc;
}

// The host inputs of a call onto workspace 0: the pool (`rows` x F doubles, room for `extra` rows behind it: the shared-id gather's
// region) into WS.hFeats and, when there is one, the association list (`assocRows` rows) into WS.hAssoc.
int upload_inputs(roman_ctx* c, const double* feats, int64_t rows, int32_t F, int64_t extra, const int32_t* assoc, int64_t assocRows,
                  const double** dFeats, const int32_t** dAssoc = nullptr)
{
    if (!feats && rows * F > 0) return fail(c, ROMAN_E_INVALID, "the pool (feats / pts) is NULL");
    HIPCHK(c, WS.hFeats.ensure(sizeof(double) * (size_t)std::max<int64_t>((rows + extra) * F, 1)));
    if (rows * F > 0) HIPCHK(c, hipMemcpyAsync(WS.hFeats.p, feats, sizeof(double) * (size_t)(rows * F), hipMemcpyHostToDevice, WS.stream));
    *dFeats = WS.hFeats.as<double>();
    if (dAssoc) *dAssoc = nullptr;
    if (assoc) {
        HIPCHK(c, WS.hAssoc.ensure(sizeof(int32_t) * 2 * (size_t)std::max<int64_t>(assocRows, 1)));
        if (assocRows > 0) HIPCHK(c, hipMemcpyAsync(WS.hAssoc.p, assoc, sizeof(int32_t) * 2 * (size_t)assocRows, hipMemcpyHostToDevice, WS.stream));
        *dAssoc = WS.hAssoc.as<int32_t>();
    }
    return ROMAN_OK;
}

// The arrays of one host-pointer stage call as ONE block of c->hostMirror.  The call declares each array once (in, out, inout, or room
// that exists on the device only); every piece is 8-byte aligned, and a piece of 0 bytes is a nullptr on the device (an optional array
// that is absent).  An inout piece goes up with the inputs, so what the device call leaves untouched comes back as it was.
struct HostMirror {
    static constexpr int CAP = 24;             // the gate, the largest call, declares 21 pieces
    enum : unsigned { UP = 1, DOWN = 2 };
    template <typename T> struct Piece {
        const HostMirror* m; int k;
        T* dev() const { return m->bytes[k] ? reinterpret_cast<T*>(m->base + m->off[k]) : nullptr; }   // valid after upload()
    };
    roman_ctx* const c;
    void* host[CAP]; size_t off[CAP], bytes[CAP]; unsigned dir[CAP];
    int n = 0; size_t total = 0; char* base = nullptr;
    explicit HostMirror(roman_ctx* c_) : c(c_) {}
    template <typename T> Piece<T> in(const T* h, size_t b) { return Piece<T>{this, add(const_cast<T*>(h), b, UP)}; }
    template <typename T> Piece<T> out(T* h, size_t b) { return Piece<T>{this, add(h, b, DOWN)}; }
    template <typename T> Piece<T> inout(T* h, size_t b) { return Piece<T>{this, add(h, b, UP | DOWN)}; }
    template <typename T> Piece<T> room(size_t b) { return Piece<T>{this, add(nullptr, b, 0)}; }
    template <typename T> Piece<T> piece(T* h, size_t b, unsigned d) { return Piece<T>{this, add(h, b, d)}; }   // the direction as data
    // the block on the device, and the in and inout pieces on their way into it
    int upload() {
        if (n > CAP) return fail(c, ROMAN_E_INTERNAL, "a host-pointer call declares more than %d arrays", CAP);
        HIPCHK(c, c->hostMirror.ensure(total));
        base = c->hostMirror.as<char>();
        for (int k = 0; k < n; ++k)
            if ((dir[k] & UP) && bytes[k]) HIPCHK(c, hipMemcpyAsync(base + off[k], host[k], bytes[k], hipMemcpyHostToDevice, WS.stream));
        return ROMAN_OK;
    }
    // the out and inout pieces back in the caller's arrays, waited for
    int download() {
        for (int k = 0; k < n; ++k)
            if ((dir[k] & DOWN) && bytes[k]) HIPCHK(c, hipMemcpyAsync(host[k], base + off[k], bytes[k], hipMemcpyDeviceToHost, WS.stream));
        HIPCHK(c, hipStreamSynchronize(WS.stream));
        return ROMAN_OK;
    }
private:
    int add(void* h, size_t b, unsigned d) {
        if (n >= CAP) { n = CAP + 1; return 0; }
        host[n] = h; off[n] = total; bytes[n] = b; dir[n] = d;
        total += (b + 7) & ~(size_t)7;
        return n++;
    }
};

// The solver's outputs of B problems as ONE block of a device buffer: T | stats | assoc | n | status
struct SolverBlock {
    int32_t kmax; size_t oT, oS, oA, oNn, oSt, end;
    SolverBlock(int32_t B, int32_t kmax_) : kmax(kmax_) {
        static_assert(sizeof(roman_stats_t) % 8 == 0, "the blocks behind the statistics stay 8-byte aligned");
        const size_t nb = (size_t)B, kb = nb * (size_t)std::max(kmax, 1);
        oT = 0; oS = oT + sizeof(double) * 16 * nb; oA = oS + sizeof(roman_stats_t) * nb;
        oNn = oA + sizeof(int32_t) * 2 * kb; oSt = oNn + sizeof(int32_t) * nb; end = oSt + sizeof(int32_t) * nb;
    }
    BatchOut at(char* dev) const {
        return BatchOut{kmax, reinterpret_cast<int32_t*>(dev + oA), reinterpret_cast<int32_t*>(dev + oNn), reinterpret_cast<double*>(dev + oT),
                        reinterpret_cast<int32_t*>(dev + oSt), reinterpret_cast<roman_stats_t*>(dev + oS)};
    }
};

// The pipeline depth a host-pointer entry point sets for its own calls (`rc`: whether that worked): every exit puts the caller's
// depth (and the team mode, which align_chunked changes) back and leaves workspace 0 on the context's stream.
struct DepthScope {
    roman_ctx* c; const int depth, teams; const int rc; bool open = true;
    DepthScope(roman_ctx* c_, int d) : c(c_), depth(c_->pipeline), teams(c_->wide_teams), rc(roman_ctx_set_pipeline(c_, d)) {}
    int close(int code) {
        if (!open) return code;
        open = false; c->wide_teams = teams;
        const int r2 = roman_ctx_set_pipeline(c, depth);
        c->cur = 0; c->ws[0].stream = c->stream;
        return code ? code : r2;
    }
    ~DepthScope() { (void)close(ROMAN_OK); }
};

// B problems as calls of `chunk`.  first_alone: the first call is waited for, so that the calls queued behind it size their pools
// from what it needed instead of repeating its guess.
template <typename Issue> int issue_chunks(roman_ctx* c, int B, int chunk, bool first_alone, Issue issue)
{
    int lo = 0;
    if (first_alone) {
        lo = std::min(B, chunk);
        int rc = issue(0, lo);
        if (!rc) rc = roman_ctx_sync(c);
        if (rc) return rc;
        harvest_totals(c, true);
    }
    for (; lo < B; lo += chunk) { const int rc = issue(lo, std::min(B, lo + chunk)); if (rc) return rc; }
    return ROMAN_OK;
}

// The flagged problems once more, in runs of consecutive problems at most a chunk long.
template <typename Flagged, typename Issue> int reissue_runs(int B, int chunk, Flagged flagged, Issue issue)
{
    for (int b = 0; b < B; ) {
        if (!flagged(b)) { ++b; continue; }
        int e = b + 1;
        while (e < B && e - b < chunk && flagged(e)) ++e;
        const int rc = issue(b, e);
        if (rc) return rc;
        b = e;
    }
    return ROMAN_OK;
}

// --- the batched hot path --------------------------------------------------------------------------
// roman_align_batch_dev, optionally with the loop-closure tail behind the solver on the same stream
int align_batch_dev(roman_ctx_t* c, const roman_params_t* params, int32_t B, const double* feats, const int64_t* off1, const int32_t* n1,
                    const int64_t* off2, const int32_t* n2, int32_t F, const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                    int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out, double* T_out, int32_t* status_out, roman_stats_t* stats_out, const LcTail* tail)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (B < 0) return fail(c, ROMAN_E_INVALID, "B < 0");
    if (B == 0) {
        if (tail) { HIPCHK(c, hipSetDevice(c->device)); return enqueue_lc_tail(c, c->stream, 0, *tail); }
        return ROMAN_OK;
    }
    if (!assoc_out || !n_assoc_out || !T_out || !status_out || kmax < 0) return fail(c, ROMAN_E_INVALID, "NULL output pointer or kmax < 0");
    BatchCheck chk; chk.assoc = assoc; chk.assoc_off = assoc_off;
    bool any = false;
    int rc = check_batch(c, B, off1, n1, off2, n2, chk, &any);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    DevParams D;
    rc = make_dev_params(c, params, F, &D);
    if (rc) return rc;
    if (!feats && any) return fail(c, ROMAN_E_INVALID, "feats is NULL");
    const BatchIn in{B, feats, off1, n1, off2, n2, F, assoc, assoc_off};
    const BatchOut out{kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out};
    return on_next_workspace(c, [&](hipStream_t stream) -> int {
        const int r = run_batch(c, D, params, in, u0, out);
        return (!r && tail) ? enqueue_lc_tail(c, stream, B, *tail) : r;
    });
}
}  // namespace

extern "C" {

int roman_align_batch_dev(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                          const double* feats, const int64_t* off1, const int32_t* n1,
                          const int64_t* off2, const int32_t* n2, int32_t F,
                          const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                          int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                          double* T_out, int32_t* status_out, roman_stats_t* stats_out)
{
    return align_batch_dev(c, params, B, feats, off1, n1, off2, n2, F, assoc, assoc_off, u0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out, nullptr);
}

// The tail on its own, on the context's stream.  At pipeline depth >= 2 the batch outputs it reads are written on internal
// streams: the caller orders them in front with roman_ctx_join().
int roman_lc_tail_dev(roman_ctx_t* c, const roman_lc_params_t* lc_params, int32_t B,
                      const double* T, const int32_t* n_assoc, const int32_t* status,
                      const double* T_ref, const int32_t* enable,
                      const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                      roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (B < 0) return fail(c, ROMAN_E_INVALID, "B < 0");
    LcTail t;
    int rc = make_lc_tail(c, lc_params, T, n_assoc, status, T_ref, enable, FL, iL, FR, iR, records, accepted_idx, n_accepted, &t);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_lc_tail(c, c->stream, B, t);
}

int roman_align_lc_batch_dev(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                          const double* feats, const int64_t* off1, const int32_t* n1,
                          const int64_t* off2, const int32_t* n2, int32_t F,
                          const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                          int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                          double* T_out, int32_t* status_out, roman_stats_t* stats_out,
                          const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                          const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                          roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (B > 0 && (!records || !accepted_idx)) return fail(c, ROMAN_E_INVALID, "records / accepted_idx is NULL");
    LcTail t;
    int rc = make_lc_tail(c, lc_params, T_out, n_assoc_out, status_out, T_ref, enable, FL, iL, FR, iR, records, accepted_idx, n_accepted, &t);
    if (rc) return rc;
    if (params && lc_params->dim != params->point_dim) return fail(c, ROMAN_E_INVALID, "lc_params.dim (%d) differs from params.point_dim (%d)", lc_params->dim, params->point_dim);
    return align_batch_dev(c, params, B, feats, off1, n1, off2, n2, F, assoc, assoc_off, u0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out, &t);
}

int roman_ctx_cosine_screen_stats(roman_ctx_t* c, int64_t* screened_batches, int64_t* dense_batches, double* latest_fallback_share)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    harvest_totals(c, false);
    if (screened_batches) *screened_batches = c->cosScreenBatches;
    if (dense_batches) *dense_batches = c->cosDenseBatches;
    if (latest_fallback_share) *latest_fallback_share = c->hist.cosSeen ? c->hist.cosDenseFrac : 0.0;
    return ROMAN_OK;
}

int roman_ctx_has_history(roman_ctx_t* c, const roman_params_t* params, int32_t F, int32_t* yes)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (!params || !yes) return fail(c, ROMAN_E_INVALID, "NULL argument");
    harvest_totals(c, false);
    const roman_ctx::Hist& H = c->hist;
    *yes = (H.valid && H.tagged && H.F == F && memcmp(&H.params, params, sizeof(roman_params_t)) == 0) ? 1 : 0;
    return ROMAN_OK;
}

int roman_ctx_set_wide_teams(roman_ctx_t* c, int teams_per_xcd)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (!(teams_per_xcd == -1 || teams_per_xcd == 0 || teams_per_xcd == 1 || teams_per_xcd == 2 || teams_per_xcd == 4))
        return fail(c, ROMAN_E_INVALID, "teams per XCD must be -1 (automatic), 0, 1, 2 or 4");
    c->wide_teams = teams_per_xcd;
    return ROMAN_OK;
}

int roman_ctx_set_host_batching(roman_ctx_t* c, int chunk, int depth)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (chunk < 1 || depth < 1 || depth > ROMAN_MAX_PIPELINE) return fail(c, ROMAN_E_INVALID, "chunk must be >= 1 and depth 1..%d", ROMAN_MAX_PIPELINE);
    c->host_chunk = chunk; c->host_depth = depth;
    return ROMAN_OK;
}

namespace {
// Attempts a problem gets before the host-pointer entry points give up on its workspace: the speculative sizes can be corrected
// once per pool (live set beyond the launch's LDS tiles / fallback kernels not launched, bit matrix, matrix slots, lists), and a
// skip the library chose itself (small_only: the general kernels left out) is one more.
constexpr int MAX_ATTEMPTS = 5;

// The host-pointer batch in CALLS of c->host_chunk problems, c->host_depth of them in flight: what the pipelined loop of a
// device-pointer caller does, for callers that hold host arrays — the straggler tail of one call's solver
// overlaps the next calls' affinity builds.  Inputs are already on the device; every call writes its own rows of the output
// arrays.  Problems a call skipped for workspace (ROMAN_ST_WORKSPACE) are issued again, those only, in runs of consecutive
// problems.  With no sizing history for this parameter block the first call runs alone and is waited for (issue_chunks).
int align_chunked(roman_ctx* c, const roman_params_t* params, const BatchIn& in, const double* dU0, const BatchOut& out)
{
    const int B = in.B, chunk = c->host_chunk;
    DepthScope scope(c, c->host_depth);
    int rc = scope.rc;
    if (rc) return rc;
    c->teams_launched = false;
    std::vector<int64_t> uoff;                                  // start of problem b's slice of u0
    if (dU0) {
        uoff.assign((size_t)B + 1, 0);
        for (int b = 0; b < B; ++b) {
            const int64_t na = in.assoc ? in.assoc_off[b + 1] - in.assoc_off[b] : 0;
            uoff[b + 1] = uoff[b] + (na > 0 ? na : (int64_t)in.n1[b] * in.n2[b]);
        }
    }
    auto issue = [&](int lo, int hi) -> int {
        return roman_align_batch_dev(c, params, hi - lo, in.feats, in.off1 + lo, in.n1 + lo, in.off2 + lo, in.n2 + lo, in.F,
                                     in.assoc, in.assoc ? in.assoc_off + lo : nullptr, dU0 ? dU0 + uoff[lo] : nullptr, out.kmax,
                                     out.assoc_out + (size_t)lo * (size_t)out.kmax * 2, out.n_assoc_out + lo, out.T_out + (size_t)lo * 16, out.status_out + lo,
                                     out.stats_out ? out.stats_out + lo : nullptr);
    };
    const roman_ctx::Hist& H = c->hist;
    const bool history = H.valid && H.tagged && H.F == in.F && memcmp(&H.params, params, sizeof(roman_params_t)) == 0;
    rc = issue_chunks(c, B, chunk, !history, issue);
    if (rc) return rc;
    std::vector<int32_t> st((size_t)B);
    bool no_teams_tried = false;
    for (int attempt = 1; ; ++attempt) {
        rc = roman_ctx_sync(c);
        if (rc) return rc;
        harvest_totals(c, true);
        if (hipMemcpy(st.data(), out.status_out, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return fail(c, ROMAN_E_HIP, "status read-back failed"); }
        int nskip = 0, nint = 0;
        for (int b = 0; b < B; ++b) { nskip += (st[b] & ROMAN_ST_WORKSPACE) ? 1 : 0; nint += (st[b] & ROMAN_ST_INTERNAL) ? 1 : 0; }
        int again = ROMAN_ST_WORKSPACE;
        if (nint && c->teams_launched && !no_teams_tried) {
            // a team of the whole-device solver that could not hold its problem leaves ROMAN_ST_INTERNAL like an expired wait does:
            // those problems once more, the whole device on one problem at a time
            no_teams_tried = true; c->wide_teams = 0; again |= ROMAN_ST_INTERNAL;
        } else if (!nskip) break;                              // nothing left to issue again (a remaining ROMAN_ST_INTERNAL is final: the caller reports it)
        // (a final ROMAN_ST_INTERNAL does not end the loop while skipped problems remain: they are still solvable)
        if (attempt >= MAX_ATTEMPTS) {
            if (!nskip) break;                                  // only the teams-off retry was pending: the ROMAN_ST_INTERNAL records speak for themselves
            return fail(c, ROMAN_E_NOMEM, "the sparse workspace of %d problem(s) still does not fit after %d attempts", nskip, attempt);
        }
        rc = reissue_runs(B, chunk, [&](int b) { return (st[b] & again) != 0; }, issue);
        if (rc) return rc;
    }
    return scope.close(ROMAN_OK);
}

// The synchronous part shared by the two host-output entry points: inputs are on the device (`in`, dU0), the outputs of every call
// land in ONE device block (T | stats | assoc | n | status) and come back with ONE copy through a pinned landing block — a single
// pair's whole result is 1.8 KB, and five separate read-backs cost more than its build kernels.
// The loop-closure tail of a host-output call: switches, its inputs already staged on the device, its outputs on the HOST.
struct LcHost {
    roman_lc_params_t P; const double* dTref; const int32_t* dEnable; const double* dFL; const int32_t* diL; const double* dFR; const int32_t* diR;
    roman_lc_record_t* records; int32_t* idx; int32_t* cnt;
};

int align_to_host(roman_ctx* c, const DevParams& D, const roman_params_t* params, const BatchIn& in, const double* dU0,
                  int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out, double* T_out, int32_t* status_out, roman_stats_t* stats_out,
                  const LcHost* lc = nullptr)
{
    const int32_t B = in.B;
    int rc = ROMAN_OK;
    bool copied = false;
    const SolverBlock blk(B, kmax);
    // with a tail: records | accepted indices | count behind the batch outputs, in the same block and the same copy
    const size_t oRec = (blk.end + 7) & ~(size_t)7, oIdx = oRec + sizeof(roman_lc_record_t) * (size_t)B, oCnt = oIdx + sizeof(int32_t) * (size_t)B;
    const size_t total = lc ? oCnt + sizeof(int32_t) : blk.end;
    static_assert(sizeof(roman_lc_record_t) % 8 == 0, "records are 8-byte aligned");
    HIPCHK(c, WS.oAll.ensure(total));
    if (c->hostOutCap < total) {
        if (c->hostOut) { (void)hipHostFree(c->hostOut); c->hostOut = nullptr; c->hostOutCap = 0; }
        const size_t want = total + total / 4 + 4096;
        HIPCHK(c, hipHostMalloc(&c->hostOut, want, hipHostMallocDefault));
        c->hostOutCap = want;
    }
    char* const dev = WS.oAll.as<char>();
    const BatchOut out = blk.at(dev);
    LcTail tail;
    if (lc) {
        tail.P = lc->P;
        tail.in = LcIn{out.T_out, out.n_assoc_out, out.status_out, lc->dTref, lc->dEnable, lc->dFL, lc->diL, lc->dFR, lc->diR};
        tail.rec = reinterpret_cast<roman_lc_record_t*>(dev + oRec); tail.idx = reinterpret_cast<int32_t*>(dev + oIdx); tail.cnt = reinterpret_cast<int32_t*>(dev + oCnt);
    }
    if (B > c->host_chunk && c->host_depth >= 2) {
        // many problems: calls of host_chunk problems, host_depth of them in flight, skipped problems issued again (align_chunked)
        rc = align_chunked(c, params, in, dU0, out);
        if (rc) return rc;
        // the tail over the FINAL device block: every re-issue has landed (align_chunked returns synchronised, on workspace 0)
        if (lc) { rc = enqueue_lc_tail(c, WS.stream, B, tail); if (rc) return rc; }
    } else
    // this entry point is synchronous anyway: when a problem did not fit the speculatively sized pools, run again
    // with the need the first attempt recorded
    {
        const int teams_saved = c->wide_teams;
        for (int attempt = 0; ; ++attempt) {
            c->teams_launched = false;
            rc = run_batch(c, D, params, in, dU0, out);
            if (!rc && lc) rc = enqueue_lc_tail(c, WS.stream, B, tail);   // behind this attempt's solver; a retry below runs it again over the new results
            if (rc) { c->wide_teams = teams_saved; return rc; }
            // the read-back rides behind the batch on the same stream: ONE wait covers both (a retry below overwrites the landing block)
            if (hipMemcpyAsync(c->hostOut, dev, total, hipMemcpyDeviceToHost, WS.stream) != hipSuccess) { (void)hipGetLastError(); c->wide_teams = teams_saved; return fail(c, ROMAN_E_HIP, "result read-back failed"); }
            if (hipStreamSynchronize(WS.stream) != hipSuccess) { (void)hipGetLastError(); c->wide_teams = teams_saved; return fail(c, ROMAN_E_HIP, "hipStreamSynchronize failed"); }
            copied = true;
            if (batch_overflowed(c)) {
                if (attempt + 1 >= MAX_ATTEMPTS) { c->wide_teams = teams_saved; return fail(c, ROMAN_E_NOMEM, "the sparse workspace still does not fit after %d attempts", attempt + 1); }
                continue;
            }
            if (c->teams_launched && c->wide_teams != 0) {      // a team that could not hold its problem leaves ROMAN_ST_INTERNAL: once more, the whole device per problem
                const int32_t* stv = reinterpret_cast<const int32_t*>(static_cast<const char*>(c->hostOut) + blk.oSt);
                bool anyInt = false;
                for (int b = 0; b < B; ++b) anyInt = anyInt || (stv[b] & ROMAN_ST_INTERNAL);
                if (anyInt && attempt + 1 < MAX_ATTEMPTS) { c->wide_teams = 0; continue; }
            }
            break;
        }
        c->wide_teams = teams_saved;
    }
    if (!copied) {
        HIPCHK(c, hipMemcpyAsync(c->hostOut, dev, total, hipMemcpyDeviceToHost, WS.stream));
        HIPCHK(c, hipStreamSynchronize(WS.stream));
    }
    {
        const char* h = static_cast<const char*>(c->hostOut);
        if (kmax > 0) memcpy(assoc_out, h + blk.oA, sizeof(int32_t) * 2 * (size_t)B * (size_t)kmax);
        memcpy(n_assoc_out, h + blk.oNn, sizeof(int32_t) * (size_t)B);
        memcpy(T_out, h + blk.oT, sizeof(double) * 16 * (size_t)B);
        memcpy(status_out, h + blk.oSt, sizeof(int32_t) * (size_t)B);
        if (stats_out) memcpy(stats_out, h + blk.oS, sizeof(roman_stats_t) * (size_t)B);
        if (lc) {
            memcpy(lc->records, h + oRec, sizeof(roman_lc_record_t) * (size_t)B);
            memcpy(lc->idx, h + oIdx, sizeof(int32_t) * (size_t)B);
            memcpy(lc->cnt, h + oCnt, sizeof(int32_t));
        }
    }
    c->last.scored = false; c->last.solved = false;
    {   // a problem the whole-device solver gave up on has no result: an error, not a quiet "0 associations"
        int nint = 0, first = -1;
        for (int b = 0; b < B; ++b) if (status_out[b] & ROMAN_ST_INTERNAL) { if (first < 0) first = b; ++nint; }
        if (nint) return fail(c, ROMAN_E_INTERNAL, "%d problem(s) reported ROMAN_ST_INTERNAL (first: %d): a bounded wait of the whole-device solver expired", nint, first);
    }
    return ROMAN_OK;
}

// --- shared-segment removal ([REF roman/align/submap_align.py:108-115]) ---------------------------------------------------------
// The problem descriptors of a call through pinned staging into c->shareDesc, behind whatever is queued on `stream`: a pure
// enqueue — only the previous call's upload out of that staging is waited for.  -> the largest map of the call.
int stage_share_descs(roman_ctx* c, hipStream_t stream, int32_t B, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t* maxN)
{
    ShareDesc* staged = nullptr;
    HIPCHK(c, c->shareStage.stage((size_t)B, &staged));
    int64_t kb = 0; int32_t m = 0;
    for (int b = 0; b < B; ++b) {
        staged[b] = ShareDesc{off1[b], off2[b], kb, n1[b], n2[b]};
        kb += (int64_t)n1[b] + n2[b];
        m = std::max(m, std::max(n1[b], n2[b]));
    }
    HIPCHK(c, c->shareStage.upload(c->shareDesc, (size_t)B, stream));
    *maxN = m;
    return ROMAN_OK;
}

// k_shared_mark behind whatever is queued on `stream`: a pure enqueue.
int enqueue_shared_mark(roman_ctx* c, hipStream_t stream, int32_t B, const int64_t* dIds, const int64_t* off1, const int32_t* n1,
                        const int64_t* off2, const int32_t* n2, int32_t* dKeep, int32_t* dKept)
{
    if (B <= 0) return ROMAN_OK;
    int32_t maxN = 0;
    const int rc = stage_share_descs(c, stream, B, off1, n1, off2, n2, &maxN);
    if (rc) return rc;
    if (maxN <= 64) hipLaunchKernelGGL(k_shared_mark<64>, dim3((unsigned)B), dim3(64), 0, stream, (int)B, c->shareDesc.as<ShareDesc>(), dIds, dKeep, dKept);
    else hipLaunchKernelGGL(k_shared_mark<256>, dim3((unsigned)B), dim3(256), 0, stream, (int)B, c->shareDesc.as<ShareDesc>(), dIds, dKeep, dKept);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// k_shared_reduce behind whatever is queued on `stream`: mark and gather in one launch, a pure enqueue.  One wave per problem
// when every map of the call has at most 64 objects, otherwise 256 threads; 16 bytes per lane when every row is 16-byte aligned.
int enqueue_shared_reduce(roman_ctx* c, hipStream_t stream, int32_t B, int32_t F, double* dFeats, int64_t region_row0, const int64_t* dIds,
                          const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t* dKeep, int32_t* dKept)
{
    if (B <= 0) return ROMAN_OK;
    int32_t maxN = 0;
    const int rc = stage_share_descs(c, stream, B, off1, n1, off2, n2, &maxN);
    if (rc) return rc;
    const bool v2 = F % 2 == 0 && reinterpret_cast<uintptr_t>(dFeats) % 16 == 0;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(dFeats);
    const ShareDesc* descs = c->shareDesc.as<ShareDesc>();
    const dim3 grid((unsigned)B);
    if (maxN <= 64) {
        if (v2) hipLaunchKernelGGL((k_shared_reduce<64, true>), grid, dim3(64), 0, stream, (int)B, (int)F, descs, dIds, dKeep, dKept, words, region_row0);
        else hipLaunchKernelGGL((k_shared_reduce<64, false>), grid, dim3(64), 0, stream, (int)B, (int)F, descs, dIds, dKeep, dKept, words, region_row0);
    } else {
        if (v2) hipLaunchKernelGGL((k_shared_reduce<256, true>), grid, dim3(256), 0, stream, (int)B, (int)F, descs, dIds, dKeep, dKept, words, region_row0);
        else hipLaunchKernelGGL((k_shared_reduce<256, false>), grid, dim3(256), 0, stream, (int)B, (int)F, descs, dIds, dKeep, dKept, words, region_row0);
    }
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// The ids of a host-pointer call and where the removal's results go (roman_align_lc_batch_ids).
struct IdsHostIn { const int64_t* ids; int32_t* n1_kept; int32_t* n2_kept; int32_t* keep; };

// The problem list after the removal: affected problems (those that lost an object on either side) point into the gather region
// behind the pool with their reduced sizes, the others are as the caller gave them.
struct ReducedProblems {
    std::vector<int64_t> off1, off2; std::vector<int32_t> n1, n2;
    std::vector<GatherJob> jobs; int64_t rows = 0; int32_t maxRows = 0;     // gather region: rows of the affected problems only
};

// Upload the ids, run the mark step, read the kept counts back (one synchronisation) and lay the gather region out on the host.
int shared_mark_host(roman_ctx* c, int32_t B, int64_t n_objects, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                     const IdsHostIn& I, ReducedProblems* R)
{
    int64_t sumN = 0;
    for (int b = 0; b < B; ++b) sumN += (int64_t)n1[b] + n2[b];
    HIPCHK(c, c->shareIds.ensure(sizeof(int64_t) * (size_t)std::max<int64_t>(n_objects, 1)));
    HIPCHK(c, c->shareKeep.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(sumN, 1)));
    HIPCHK(c, c->shareKept.ensure(sizeof(int32_t) * 2 * (size_t)B));
    if (n_objects > 0) HIPCHK(c, hipMemcpyAsync(c->shareIds.p, I.ids, sizeof(int64_t) * (size_t)n_objects, hipMemcpyHostToDevice, WS.stream));
    int rc = enqueue_shared_mark(c, WS.stream, B, c->shareIds.as<int64_t>(), off1, n1, off2, n2, c->shareKeep.as<int32_t>(), c->shareKept.as<int32_t>());
    if (rc) return rc;
    std::vector<int32_t> kv((size_t)B * 2);
    HIPCHK(c, hipMemcpyAsync(kv.data(), c->shareKept.p, sizeof(int32_t) * 2 * (size_t)B, hipMemcpyDeviceToHost, WS.stream));
    if (I.keep && sumN > 0) HIPCHK(c, hipMemcpyAsync(I.keep, c->shareKeep.p, sizeof(int32_t) * (size_t)sumN, hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    R->off1.assign(off1, off1 + B); R->off2.assign(off2, off2 + B); R->n1.assign(n1, n1 + B); R->n2.assign(n2, n2 + B);
    int64_t kb = 0, g = n_objects;
    for (int b = 0; b < B; ++b) {
        const int32_t k1 = kv[2 * (size_t)b], k2 = kv[2 * (size_t)b + 1];
        if (k1 < 0 || k1 > n1[b] || k2 < 0 || k2 > n2[b]) return fail(c, ROMAN_E_HIP, "problem %d: the mark step reported %d / %d kept of %d / %d objects", b, k1, k2, n1[b], n2[b]);
        I.n1_kept[b] = k1; I.n2_kept[b] = k2;
        if (k1 != n1[b] || k2 != n2[b]) {
            if (k1 > 0) R->jobs.push_back(GatherJob{off1[b], g, kb, k1, 0});
            R->off1[b] = g; R->n1[b] = k1; g += k1;
            if (k2 > 0) R->jobs.push_back(GatherJob{off2[b], g, kb + n1[b], k2, 0});
            R->off2[b] = g; R->n2[b] = k2; g += k2;
            R->maxRows = std::max(R->maxRows, std::max(k1, k2));
        }
        kb += (int64_t)n1[b] + n2[b];
    }
    R->rows = g - n_objects;
    return ROMAN_OK;
}

// k_shared_gather: the kept rows of the affected problems into the gather region behind the pool (dFeats holds pool + region).
int enqueue_shared_gather(roman_ctx* c, hipStream_t stream, int32_t F, const ReducedProblems& R, double* dFeats)
{
    if (R.jobs.empty() || F <= 0) return ROMAN_OK;
    if (R.jobs.size() > (size_t)0x7fffffff) return fail(c, ROMAN_E_TOO_LARGE, "too many problems lost shared segments for one gather launch");
    HIPCHK(c, c->shareJobs.ensure(sizeof(GatherJob) * R.jobs.size()));
    HIPCHK(c, hipMemcpyAsync(c->shareJobs.p, R.jobs.data(), sizeof(GatherJob) * R.jobs.size(), hipMemcpyHostToDevice, stream));
    const dim3 grid((unsigned)R.jobs.size(), (unsigned)std::min(8, std::max(1, (R.maxRows + 3) / 4)));
    unsigned long long* pool = reinterpret_cast<unsigned long long*>(dFeats);
    if (F % 2 == 0) hipLaunchKernelGGL(k_shared_gather<true>, grid, dim3(256), 0, stream, (int)F, c->shareJobs.as<GatherJob>(), c->shareKeep.as<int32_t>(), pool);
    else hipLaunchKernelGGL(k_shared_gather<false>, grid, dim3(256), 0, stream, (int)F, c->shareJobs.as<GatherJob>(), c->shareKeep.as<int32_t>(), pool);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// The host arrays of the tail of roman_align_lc_batch (checked and staged behind the batch inputs).
struct LcHostIn {
    const roman_lc_params_t* P; const double* T_ref; const int32_t* enable; const double* FL; int32_t n_left; const int32_t* iL;
    const double* FR; int32_t n_right; const int32_t* iR; roman_lc_record_t* records; int32_t* idx; int32_t* cnt;
};

int align_batch_host(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                      const double* feats, int64_t n_objects,
                      const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t F,
                      const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                      int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                      double* T_out, int32_t* status_out, roman_stats_t* stats_out, const LcHostIn* lci, const IdsHostIn* idh = nullptr)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (B < 0 || n_objects < 0 || F < 0) return fail(c, ROMAN_E_INVALID, "negative size");
    if (idh) {
        if (assoc) return fail(c, ROMAN_E_INVALID, "explicit association lists cannot be combined with the removal of shared ids (they would index the lists before the removal): assoc must be NULL");
        if (!idh->ids && n_objects > 0) return fail(c, ROMAN_E_INVALID, "ids is NULL");
        if (B > 0 && (!idh->n1_kept || !idh->n2_kept)) return fail(c, ROMAN_E_INVALID, "n1_kept / n2_kept is NULL");
    }
    if (lci) {
        int rc0 = check_lc_params(c, lci->P);
        if (rc0) return rc0;
        if (!lci->cnt) return fail(c, ROMAN_E_INVALID, "n_accepted is NULL");
        if (B > 0 && (!lci->records || !lci->idx)) return fail(c, ROMAN_E_INVALID, "records / accepted_idx is NULL");
        if ((lci->FL != nullptr) != (lci->iL != nullptr) || (lci->FR != nullptr) != (lci->iR != nullptr)) return fail(c, ROMAN_E_INVALID, "a frame pool and its index array come together (FL with iL, FR with iR)");
        if (params && lci->P->dim != params->point_dim) return fail(c, ROMAN_E_INVALID, "lc_params.dim (%d) differs from params.point_dim (%d)", lci->P->dim, params->point_dim);
        for (int b = 0; b < B; ++b) {                            // the device indexes the frame pools with these
            if (lci->iL && (lci->iL[b] < 0 || lci->iL[b] >= lci->n_left)) return fail(c, ROMAN_E_INVALID, "iL[%d] = %d outside the %d left frames", b, lci->iL[b], lci->n_left);
            if (lci->iR && (lci->iR[b] < 0 || lci->iR[b] >= lci->n_right)) return fail(c, ROMAN_E_INVALID, "iR[%d] = %d outside the %d right frames", b, lci->iR[b], lci->n_right);
        }
        if (B == 0) { *lci->cnt = 0; return ROMAN_OK; }
    }
    if (B == 0) return ROMAN_OK;
    if (!assoc_out || !n_assoc_out || !T_out || !status_out || kmax < 0) return fail(c, ROMAN_E_INVALID, "NULL output pointer or kmax < 0");
    BatchCheck chk; chk.n_objects = n_objects; chk.assoc = assoc; chk.assoc_off = assoc_off; chk.assoc_on_host = true; chk.whole_list = true;
    int rc = check_batch(c, B, off1, n1, off2, n2, chk);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    DevParams D;
    rc = make_dev_params(c, params, F, &D);
    if (rc) return rc;
    int64_t sumA = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t na = assoc ? (assoc_off[b + 1] - assoc_off[b]) : 0;
        sumA += na > 0 ? na : (int64_t)n1[b] * n2[b];      // an empty list means all-to-all
    }
    ReducedProblems red;
    if (idh) {
        // mark, read the kept counts back, size the gather region: from here on the problems are the reduced ones
        rc = shared_mark_host(c, B, n_objects, off1, n1, off2, n2, *idh, &red);
        if (rc) return rc;
        off1 = red.off1.data(); n1 = red.n1.data(); off2 = red.off2.data(); n2 = red.n2.data();
        sumA = 0;
        for (int b = 0; b < B; ++b) sumA += (int64_t)n1[b] * n2[b];
    }
    const double* dFeats = nullptr; const int32_t* dA = nullptr;
    rc = upload_inputs(c, feats, n_objects, F, red.rows /* the rows of the affected problems, behind the pool */, assoc, assoc ? assoc_off[B] : 0, &dFeats, &dA);
    if (rc) return rc;
    if (idh) { rc = enqueue_shared_gather(c, WS.stream, F, red, WS.hFeats.as<double>()); if (rc) return rc; }
    const double* dU0 = nullptr;
    if (u0) {
        HIPCHK(c, WS.hU0.ensure(sizeof(double) * (size_t)std::max<int64_t>(sumA, 1)));
        if (sumA > 0) HIPCHK(c, hipMemcpyAsync(WS.hU0.p, u0, sizeof(double) * (size_t)sumA, hipMemcpyHostToDevice, WS.stream));
        dU0 = WS.hU0.as<double>();
    }
    const BatchIn in{B, dFeats, off1, n1, off2, n2, F, dA, assoc_off};
    if (!lci) return align_to_host(c, D, params, in, dU0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out);
    // the tail's inputs in one staging block: doubles first (T_ref | FL | FR), then the int32 arrays (enable | iL | iR)
    const size_t nRef = lci->T_ref ? (size_t)B * 16 : 0, nFL = lci->FL ? (size_t)lci->n_left * 16 : 0, nFR = lci->FR ? (size_t)lci->n_right * 16 : 0;
    const size_t oFL = sizeof(double) * nRef, oFR = oFL + sizeof(double) * nFL, oEn = oFR + sizeof(double) * nFR;
    const size_t oIL = oEn + (lci->enable ? sizeof(int32_t) * (size_t)B : 0), oIR = oIL + (lci->iL ? sizeof(int32_t) * (size_t)B : 0);
    const size_t stageBytes = oIR + (lci->iR ? sizeof(int32_t) * (size_t)B : 0);
    HIPCHK(c, WS.lcStage.ensure(std::max<size_t>(stageBytes, 8)));
    char* const sd = WS.lcStage.as<char>();
    auto up = [&](size_t off, const void* src, size_t bytes) -> hipError_t { return bytes ? hipMemcpyAsync(sd + off, src, bytes, hipMemcpyHostToDevice, WS.stream) : hipSuccess; };
    HIPCHK(c, up(0, lci->T_ref, sizeof(double) * nRef));
    HIPCHK(c, up(oFL, lci->FL, sizeof(double) * nFL));
    HIPCHK(c, up(oFR, lci->FR, sizeof(double) * nFR));
    HIPCHK(c, up(oEn, lci->enable, lci->enable ? sizeof(int32_t) * (size_t)B : 0));
    HIPCHK(c, up(oIL, lci->iL, lci->iL ? sizeof(int32_t) * (size_t)B : 0));
    HIPCHK(c, up(oIR, lci->iR, lci->iR ? sizeof(int32_t) * (size_t)B : 0));
    LcHost lh;
    lh.P = *lci->P;
    lh.dTref = lci->T_ref ? reinterpret_cast<const double*>(sd) : nullptr;
    lh.dFL = lci->FL ? reinterpret_cast<const double*>(sd + oFL) : nullptr;
    lh.dFR = lci->FR ? reinterpret_cast<const double*>(sd + oFR) : nullptr;
    lh.dEnable = lci->enable ? reinterpret_cast<const int32_t*>(sd + oEn) : nullptr;
    lh.diL = lci->iL ? reinterpret_cast<const int32_t*>(sd + oIL) : nullptr;
    lh.diR = lci->iR ? reinterpret_cast<const int32_t*>(sd + oIR) : nullptr;
    lh.records = lci->records; lh.idx = lci->idx; lh.cnt = lci->cnt;
    return align_to_host(c, D, params, in, dU0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out, &lh);
}
}  // namespace

int roman_align_batch(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                      const double* feats, int64_t n_objects,
                      const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t F,
                      const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                      int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                      double* T_out, int32_t* status_out, roman_stats_t* stats_out)
{
    return align_batch_host(c, params, B, feats, n_objects, off1, n1, off2, n2, F, assoc, assoc_off, u0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out, nullptr);
}

int roman_align_lc_batch(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                      const double* feats, int64_t n_objects,
                      const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t F,
                      const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                      int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                      double* T_out, int32_t* status_out, roman_stats_t* stats_out,
                      const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                      const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                      roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted)
{
    const LcHostIn lci{lc_params, T_ref, enable, FL, n_left, iL, FR, n_right, iR, records, accepted_idx, n_accepted};
    return align_batch_host(c, params, B, feats, n_objects, off1, n1, off2, n2, F, assoc, assoc_off, u0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out, &lci);
}

/* roman_align_lc_batch with the shared-segment removal of single-robot loop closures in front
   ([REF roman/align/submap_align.py:108-115]): every submap is uploaded once, the removal runs on the device. */
int roman_align_lc_batch_ids(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                      const double* feats, int64_t n_objects,
                      const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t F,
                      const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                      int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                      double* T_out, int32_t* status_out, roman_stats_t* stats_out,
                      const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                      const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                      roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted,
                      const int64_t* ids, int32_t* n1_kept, int32_t* n2_kept, int32_t* keep)
{
    const LcHostIn lci{lc_params, T_ref, enable, FL, n_left, iL, FR, n_right, iR, records, accepted_idx, n_accepted};
    const IdsHostIn idh{ids, n1_kept, n2_kept, keep};
    return align_batch_host(c, params, B, feats, n_objects, off1, n1, off2, n2, F, assoc, assoc_off, u0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out, &lci, &idh);
}

/* The mark step alone on the context's stream, all bulk pointers DEVICE: a pure enqueue. */
int roman_shared_ids_dev(roman_ctx_t* c, int32_t B, const int64_t* ids, const int64_t* off1, const int32_t* n1,
                         const int64_t* off2, const int32_t* n2, int32_t* keep, int32_t* kept)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (B < 0) return fail(c, ROMAN_E_INVALID, "B < 0");
    if (B == 0) return ROMAN_OK;
    if (!kept) return fail(c, ROMAN_E_INVALID, "NULL output pointer");
    bool any = false;
    const int rc = check_batch(c, B, off1, n1, off2, n2, BatchCheck{}, &any);
    if (rc) return rc;
    if (any && (!ids || !keep)) return fail(c, ROMAN_E_INVALID, "ids / keep is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_shared_mark(c, c->stream, B, ids, off1, n1, off2, n2, keep, kept);
}

/* Mark and gather in one launch on the context's stream, all bulk pointers DEVICE: a pure enqueue. */
int roman_shared_reduce_dev(roman_ctx_t* c, int32_t B, int32_t F, double* feats, int64_t region_row0, const int64_t* ids,
                            const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t* keep, int32_t* kept)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (B < 0) return fail(c, ROMAN_E_INVALID, "B < 0");
    if (F < 1) return fail(c, ROMAN_E_INVALID, "F = %d: a row has at least one column", F);
    if (region_row0 < 0) return fail(c, ROMAN_E_INVALID, "region_row0 < 0");
    if (B == 0) return ROMAN_OK;
    if (!kept) return fail(c, ROMAN_E_INVALID, "kept is NULL");
    bool any = false;
    BatchCheck chk; chk.n_objects = region_row0;                 // the pool slices lie in front of the gather region
    const int rc = check_batch(c, B, off1, n1, off2, n2, chk, &any);
    if (rc) return rc;
    if (any && (!feats || !ids || !keep)) return fail(c, ROMAN_E_INVALID, "feats / ids / keep is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_shared_reduce(c, c->stream, B, F, feats, region_row0, ids, off1, n1, off2, n2, keep, kept);
}

/* roman_align_batch_resident: inputs in HBM (as roman_align_batch_dev), results on the HOST (as roman_align_batch). */
int roman_align_batch_resident(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                               const double* feats, const int64_t* off1, const int32_t* n1,
                               const int64_t* off2, const int32_t* n2, int32_t F,
                               const int32_t* assoc, const int64_t* assoc_off, const double* u0,
                               int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                               double* T_out, int32_t* status_out, roman_stats_t* stats_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (B < 0 || F < 0) return fail(c, ROMAN_E_INVALID, "negative size");
    if (B == 0) return ROMAN_OK;
    if (!assoc_out || !n_assoc_out || !T_out || !status_out || kmax < 0) return fail(c, ROMAN_E_INVALID, "NULL output pointer or kmax < 0");
    BatchCheck chk; chk.assoc = assoc; chk.assoc_off = assoc_off; chk.whole_list = true;
    bool any = false;
    int rc = check_batch(c, B, off1, n1, off2, n2, chk, &any);
    if (rc) return rc;
    if (!feats && any) return fail(c, ROMAN_E_INVALID, "feats is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    DevParams D;
    rc = make_dev_params(c, params, F, &D);
    if (rc) return rc;
    const BatchIn in{B, feats, off1, n1, off2, n2, F, assoc, assoc_off};
    return align_to_host(c, D, params, in, u0, kmax, assoc_out, n_assoc_out, T_out, status_out, stats_out);
}

// --- multi-solution extraction, batched ([REF roman/align/object_registration.py:57-86]) ------------------------------------------
// The rounds of one call on workspace c->cur and its stream (pure enqueue): the batch is scored once into the stream layout as the
// plain-CLIPPER view (every input association a node, unit diagonal), then per round the stream solver runs on the current values
// and k_mno_round scores the selection on the unmasked values, files the solution and zeroes the selected block in the copy the
// next solve reads (WS.vals stays as scored; WS.mnoVals is the masked copy, made by the first round's pass).
static int run_mno(roman_ctx* c, const DevParams& D0, const roman_params_t* params, const BatchIn& in, int32_t K, int32_t kmax,
                   int32_t* assoc_out, roman_mno_solution_t* sol_out, roman_stats_t* stats_out)
{
    const int B = in.B;
    DevParams Dv = D0;
    const int diagOne = (!D0.single || D0.diag_one) ? 1 : 0;    // the diagonal of M as exported: 1, or the single scores (k_live leaves them in ls)
    if (Dv.single && !Dv.pruned) { Dv.plain_all = 1; Dv.diag_one = 1; }   // (the pruned prefilter's survivors ARE the list clipperpy is handed: already plain)
    // the view's pools are sized by a history of its own: tagged with a parameter block no caller can pass (reserved != 0)
    roman_params_t tag = *params; tag.reserved = 0x4d4e4f;
    std::vector<ProbDesc> hd;
    DevParams D;
    int rc = enqueue_score(c, Dv, &tag, in, hd, &D, nullptr, nullptr, true);
    if (rc) return rc;
    int64_t sumA = 0, maxA = 0; for (const ProbDesc& d : hd) { sumA += d.nA; maxA = std::max<int64_t>(maxA, d.nA); }
    // the solver's block of one round: T | stats | assoc | n | status
    const SolverBlock blk(B, kmax);
    HIPCHK(c, WS.mnoOut.ensure(blk.end));
    if (K > 1) HIPCHK(c, WS.mnoVals.ensure(sizeof(double) * (size_t)std::max<long long>(WS.capNnz, 1)));
    const BatchOut out = blk.at(WS.mnoOut.as<char>());
    for (int r = 0; r < K && !rc; ++r) {
        if (r > 0) std::swap(WS.vals, WS.mnoVals);              // this round's solve reads the masked copy
        rc = enqueue_solve(c, D, B, sumA, maxA, in.feats, in.assoc, nullptr, false, 0, out);
        if (r > 0) std::swap(WS.vals, WS.mnoVals);
        if (rc) break;
        MnoRound R;
        R.n_assoc = out.n_assoc_out; R.status = out.status_out; R.T = out.T_out; R.stats = out.stats_out; R.assoc = out.assoc_out;
        R.assoc_out = assoc_out; R.sol_out = sol_out; R.stats_out = stats_out;
        R.K = K; R.r = r; R.kmax = kmax; R.maskMode = (r + 1 >= K) ? 0 : (r == 0 ? 1 : 2); R.diagOne = diagOne;
        hipLaunchKernelGGL(k_mno_round, dim3((unsigned)B), dim3(MNO_NT), 0, WS.stream, B, R, WS.probs.as<ProbDesc>(), WS.state.as<ProbState>(),
                           WS.lp.as<int32_t>(), WS.ls.as<double>(), WS.rowPos.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.cols16.as<uint16_t>(),
                           WS.vals.as<double>(), K > 1 ? WS.mnoVals.as<double>() : (double*)nullptr,
                           WS.nodesOrig.as<int32_t>(), WS.nSel.as<int32_t>(), WS.uOut.as<double>());
        HIPCHK(c, hipGetLastError());
        DBG(c, "k_mno_round");
    }
    return rc;
}

static int mno_check(roman_ctx* c, const roman_params_t* params, int32_t B, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                     const BatchCheck& chk, int32_t K, int32_t kmax, const void* assoc_out, const void* sol_out, bool* any = nullptr)
{
    if (B < 0) return fail(c, ROMAN_E_INVALID, "B < 0");
    if (K < 1 || K > ROMAN_MNO_MAX_SOLUTIONS) return fail(c, ROMAN_E_INVALID, "num_solutions must be 1..%d (got %d)", ROMAN_MNO_MAX_SOLUTIONS, K);
    if (B == 0) return ROMAN_OK;
    if (!params) return fail(c, ROMAN_E_INVALID, "params is NULL");
    if (!assoc_out || !sol_out || kmax < 0) return fail(c, ROMAN_E_INVALID, "NULL output pointer or kmax < 0");
    const int rc = check_batch(c, B, off1, n1, off2, n2, chk, any);
    if (rc) return rc;
    if (params->maxiniters < 1 || params->maxlsiters < 1) return fail(c, ROMAN_E_UNSUPPORTED, "roman_mno_batch needs maxiniters >= 1 and maxlsiters >= 1");
    for (int b = 0; b < B; ++b) {
        const int64_t nl = chk.assoc ? chk.assoc_off[b + 1] - chk.assoc_off[b] : 0;
        const int64_t na = nl > 0 ? nl : (int64_t)n1[b] * n2[b];
        if (na > ROMAN_MNO_MAX_ASSOC) return fail(c, ROMAN_E_TOO_LARGE, "problem %d has %lld associations; roman_mno_batch serves at most %d per problem", b, (long long)na, ROMAN_MNO_MAX_ASSOC);
    }
    return ROMAN_OK;
}

// The tail over K hypotheses per problem: switches, device inputs, device outputs.
struct MnoLcTail {
    roman_lc_params_t P; const double* T_ref; const int32_t* enable; const double* FL; const int32_t* iL; const double* FR; const int32_t* iR;
    roman_lc_record_t* rec; int32_t* best; int32_t* idx; int32_t* cnt; int32_t* bidx; int32_t* bcnt;
};

static int make_mno_lc_tail(roman_ctx* c, const roman_lc_params_t* lp, int32_t B, int32_t K, const double* T_ref, const int32_t* enable,
                            const double* FL, const int32_t* iL, const double* FR, const int32_t* iR, roman_lc_record_t* records, int32_t* best,
                            int32_t* accepted_idx, int32_t* n_accepted, int32_t* accepted_best_idx, int32_t* n_accepted_best, MnoLcTail* t)
{
    if (B < 0) return fail(c, ROMAN_E_INVALID, "B < 0");
    if (K < 1 || K > ROMAN_MNO_MAX_SOLUTIONS) return fail(c, ROMAN_E_INVALID, "num_solutions must be 1..%d (got %d)", ROMAN_MNO_MAX_SOLUTIONS, K);
    if ((int64_t)B * K > INT32_MAX) return fail(c, ROMAN_E_INVALID, "B * num_solutions = %lld records: a record index is an int32", (long long)B * K);
    const int rc = check_lc_params(c, lp);
    if (rc) return rc;
    if (!n_accepted || !n_accepted_best) return fail(c, ROMAN_E_INVALID, "n_accepted / n_accepted_best is NULL");
    if ((FL != nullptr) != (iL != nullptr) || (FR != nullptr) != (iR != nullptr)) return fail(c, ROMAN_E_INVALID, "a frame pool and its index array come together (FL with iL, FR with iR)");
    if (B > 0 && (!records || !best)) return fail(c, ROMAN_E_INVALID, "records / best is NULL");
    if (B > 0 && (!accepted_idx || !accepted_best_idx)) return fail(c, ROMAN_E_INVALID, "accepted_idx / accepted_best_idx is NULL");
    *t = MnoLcTail{*lp, T_ref, enable, FL, iL, FR, iR, records, best, accepted_idx, n_accepted, accepted_best_idx, n_accepted_best};
    return ROMAN_OK;
}

// k_mno_lc_tail, then both lists, behind whatever is queued on `stream`
static int enqueue_mno_lc_tail(roman_ctx* c, hipStream_t stream, int B, int K, const roman_mno_solution_t* sol, const MnoLcTail& t)
{
    if (B > 0) {
        if (!sol) return fail(c, ROMAN_E_INVALID, "sol is NULL");
        constexpr int PER = MNO_LC_NT / 64;
        hipLaunchKernelGGL(k_mno_lc_tail, dim3((unsigned)((B + PER - 1) / PER)), dim3(MNO_LC_NT), 0, stream, t.P, (int)B, (int)K, sol,
                           t.T_ref, t.enable, t.FL, t.iL, t.FR, t.iR, t.rec, t.best);
        HIPCHK(c, hipGetLastError());
    }
    const int n = B * K;
    hipLaunchKernelGGL(k_lc_compact, dim3(1), dim3(n > 256 ? 1024 : 256), 0, stream, n, (const roman_lc_record_t*)t.rec, t.idx, t.cnt);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_mno_best_compact, dim3(1), dim3(B > 256 ? 1024 : 256), 0, stream, (int)B, (int)K, (const roman_lc_record_t*)t.rec,
                       (const int32_t*)t.best, t.bidx, t.bcnt);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// roman_mno_batch_dev, optionally with the hypothesis tail behind the last round on the same stream
static int mno_batch_dev(roman_ctx_t* c, const roman_params_t* params, int32_t B, const double* feats, const int64_t* off1, const int32_t* n1,
                         const int64_t* off2, const int32_t* n2, int32_t F, const int32_t* assoc, const int64_t* assoc_off,
                         int32_t num_solutions, int32_t kmax, int32_t* assoc_out, roman_mno_solution_t* sol_out, roman_stats_t* stats_out,
                         const MnoLcTail* tail)
{
    BatchCheck chk; chk.assoc = assoc; chk.assoc_off = assoc_off;
    bool any = false;
    int rc = mno_check(c, params, B, off1, n1, off2, n2, chk, num_solutions, kmax, assoc_out, sol_out, &any);
    if (rc) return rc;
    if (B == 0) {
        if (tail) { HIPCHK(c, hipSetDevice(c->device)); return enqueue_mno_lc_tail(c, c->stream, 0, num_solutions, nullptr, *tail); }
        return ROMAN_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    DevParams D;
    rc = make_dev_params(c, params, F, &D);
    if (rc) return rc;
    if (!feats && any) return fail(c, ROMAN_E_INVALID, "feats is NULL");
    static_assert(STREAM_MAXL == ROMAN_MNO_MAX_ASSOC, "the documented cap is the stream layout's");
    const BatchIn in{B, feats, off1, n1, off2, n2, F, assoc, assoc_off};
    return on_next_workspace(c, [&](hipStream_t stream) -> int {
        const int r = run_mno(c, D, params, in, num_solutions, kmax, assoc_out, sol_out, stats_out);
        return (!r && tail) ? enqueue_mno_lc_tail(c, stream, B, num_solutions, sol_out, *tail) : r;
    });
}

int roman_mno_batch_dev(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                        const double* feats, const int64_t* off1, const int32_t* n1,
                        const int64_t* off2, const int32_t* n2, int32_t F,
                        const int32_t* assoc, const int64_t* assoc_off,
                        int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                        roman_mno_solution_t* sol_out, roman_stats_t* stats_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    return mno_batch_dev(c, params, B, feats, off1, n1, off2, n2, F, assoc, assoc_off, num_solutions, kmax, assoc_out, sol_out, stats_out, nullptr);
}

// The hypothesis tail on its own, on the context's stream.  At pipeline depth >= 2 the solutions it reads are written on internal
// streams: the caller orders them in front with roman_ctx_join().
int roman_mno_lc_tail_dev(roman_ctx_t* c, const roman_lc_params_t* lc_params, int32_t B, int32_t K, const roman_mno_solution_t* sol,
                          const double* T_ref, const int32_t* enable, const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                          roman_lc_record_t* records, int32_t* best, int32_t* accepted_idx, int32_t* n_accepted,
                          int32_t* accepted_best_idx, int32_t* n_accepted_best)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    MnoLcTail t;
    const int rc = make_mno_lc_tail(c, lc_params, B, K, T_ref, enable, FL, iL, FR, iR, records, best, accepted_idx, n_accepted, accepted_best_idx, n_accepted_best, &t);
    if (rc) return rc;
    if (B > 0 && !sol) return fail(c, ROMAN_E_INVALID, "sol is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_mno_lc_tail(c, c->stream, B, K, sol, t);
}

int roman_mno_lc_batch_dev(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                           const double* feats, const int64_t* off1, const int32_t* n1,
                           const int64_t* off2, const int32_t* n2, int32_t F,
                           const int32_t* assoc, const int64_t* assoc_off,
                           int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                           roman_mno_solution_t* sol_out, roman_stats_t* stats_out,
                           const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                           const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                           roman_lc_record_t* records, int32_t* best, int32_t* accepted_idx, int32_t* n_accepted,
                           int32_t* accepted_best_idx, int32_t* n_accepted_best)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    MnoLcTail t;
    const int rc = make_mno_lc_tail(c, lc_params, B, num_solutions, T_ref, enable, FL, iL, FR, iR, records, best, accepted_idx, n_accepted, accepted_best_idx, n_accepted_best, &t);
    if (rc) return rc;
    if (params && lc_params->dim != params->point_dim) return fail(c, ROMAN_E_INVALID, "lc_params.dim (%d) differs from params.point_dim (%d)", lc_params->dim, params->point_dim);
    return mno_batch_dev(c, params, B, feats, off1, n1, off2, n2, F, assoc, assoc_off, num_solutions, kmax, assoc_out, sol_out, stats_out, &t);
}

// What roman_mno_lc_batch adds to roman_mno_batch: the tail's host arrays.
struct MnoLcHost {
    const roman_lc_params_t* lp; const double* T_ref; const int32_t* enable; const double* FL; int32_t n_left; const int32_t* iL;
    const double* FR; int32_t n_right; const int32_t* iR; roman_lc_record_t* records; int32_t* best; int32_t* accepted_idx; int32_t* n_accepted;
    int32_t* accepted_best_idx; int32_t* n_accepted_best;
};

static int mno_to_host(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                       const double* feats, int64_t n_objects,
                       const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t F,
                       const int32_t* assoc, const int64_t* assoc_off,
                       int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                       roman_mno_solution_t* sol_out, roman_stats_t* stats_out, const MnoLcHost* lc)
{
    if (n_objects < 0 || F < 0) return fail(c, ROMAN_E_INVALID, "negative size");
    BatchCheck chk; chk.n_objects = n_objects; chk.assoc = assoc; chk.assoc_off = assoc_off; chk.assoc_on_host = true; chk.whole_list = true;
    int rc = mno_check(c, params, B, off1, n1, off2, n2, chk, num_solutions, kmax, assoc_out, sol_out);
    if (rc) return rc;
    if (B == 0) { if (lc) { *lc->n_accepted = 0; *lc->n_accepted_best = 0; } return ROMAN_OK; }
    const int K = num_solutions;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    { DevParams Dchk; rc = make_dev_params(c, params, F, &Dchk); if (rc) return rc; }
    const double* dFeats = nullptr; const int32_t* dA = nullptr;
    rc = upload_inputs(c, feats, n_objects, F, 0, assoc, assoc ? assoc_off[B] : 0, &dFeats, &dA);
    if (rc) return rc;
    // outputs on the device: solutions | statistics | association rows
    const size_t nSol = (size_t)B * (size_t)K, rowsPer = (size_t)std::max(kmax, 0) * 2;
    const size_t oSol = 0, oStats = oSol + sizeof(roman_mno_solution_t) * nSol, oAssoc = oStats + sizeof(roman_stats_t) * nSol,
                 total = oAssoc + sizeof(int32_t) * nSol * std::max<size_t>(rowsPer, 1);
    static_assert(sizeof(roman_mno_solution_t) % 8 == 0 && sizeof(roman_stats_t) % 8 == 0, "the blocks stay 8-byte aligned");
    HIPCHK(c, WS.mnoHost.ensure(total));
    char* const dev = WS.mnoHost.as<char>();
    roman_mno_solution_t* dSol = reinterpret_cast<roman_mno_solution_t*>(dev + oSol);
    roman_stats_t* dStats = reinterpret_cast<roman_stats_t*>(dev + oStats);
    int32_t* dAssoc = reinterpret_cast<int32_t*>(dev + oAssoc);
    // calls of host_chunk problems, host_depth of them in flight; skipped problems are issued again, those only
    const int chunk = std::max(1, c->host_chunk);
    DepthScope scope(c, B > chunk ? c->host_depth : 1);
    if (scope.rc) return scope.rc;
    auto issue = [&](int lo, int hi) -> int {
        return roman_mno_batch_dev(c, params, hi - lo, dFeats, off1 + lo, n1 + lo, off2 + lo, n2 + lo, F, dA, dA ? assoc_off + lo : nullptr, K, kmax,
                                   dAssoc + (size_t)lo * (size_t)K * rowsPer, dSol + (size_t)lo * (size_t)K, dStats + (size_t)lo * (size_t)K);
    };
    rc = issue_chunks(c, B, chunk, c->pipeline >= 2, issue);
    if (rc) return rc;
    std::vector<roman_mno_solution_t> hs(nSol);
    for (int attempt = 1; ; ++attempt) {
        rc = roman_ctx_sync(c);
        if (rc) return rc;
        harvest_totals(c, true);
        if (hipMemcpy(hs.data(), dSol, sizeof(roman_mno_solution_t) * nSol, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return fail(c, ROMAN_E_HIP, "solution read-back failed"); }
        auto skipped = [&](int b) { return (hs[(size_t)b * K].status & ROMAN_ST_WORKSPACE) != 0; };
        int nskip = 0;
        for (int b = 0; b < B; ++b) nskip += skipped(b) ? 1 : 0;
        if (!nskip) break;
        if (attempt >= MAX_ATTEMPTS) return fail(c, ROMAN_E_NOMEM, "the sparse workspace of %d problem(s) still does not fit after %d attempts", nskip, attempt);
        rc = reissue_runs(B, chunk, skipped, issue);
        if (rc) return rc;
    }
    memcpy(sol_out, hs.data(), sizeof(roman_mno_solution_t) * nSol);
    if (stats_out && hipMemcpy(stats_out, dStats, sizeof(roman_stats_t) * nSol, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return fail(c, ROMAN_E_HIP, "statistics read-back failed"); }
    if (rowsPer && hipMemcpy(assoc_out, dAssoc, sizeof(int32_t) * nSol * rowsPer, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return fail(c, ROMAN_E_HIP, "association read-back failed"); }
    if (lc) {                                                    // the tail ONCE over the final block: no record comes from a skipped attempt
        const size_t nb = (size_t)B;
        HostMirror m(c);
        const auto dRef = m.in(lc->T_ref, lc->T_ref ? sizeof(double) * 16 * nb : 0);
        const auto dEn = m.in(lc->enable, lc->enable ? sizeof(int32_t) * nb : 0);
        const auto dFL = m.in(lc->FL, lc->FL ? sizeof(double) * 16 * (size_t)lc->n_left : 0);
        const auto dIL = m.in(lc->iL, lc->iL ? sizeof(int32_t) * nb : 0);
        const auto dFR = m.in(lc->FR, lc->FR ? sizeof(double) * 16 * (size_t)lc->n_right : 0);
        const auto dIR = m.in(lc->iR, lc->iR ? sizeof(int32_t) * nb : 0);
        const auto lrec = m.out(lc->records, sizeof(roman_lc_record_t) * nSol);
        const auto lbest = m.out(lc->best, sizeof(int32_t) * nb);
        const auto lidx = m.out(lc->accepted_idx, sizeof(int32_t) * nSol);
        const auto lcnt = m.out(lc->n_accepted, sizeof(int32_t));
        const auto bidx = m.out(lc->accepted_best_idx, sizeof(int32_t) * nb);
        const auto bcnt = m.out(lc->n_accepted_best, sizeof(int32_t));
        rc = m.upload();
        if (rc) return rc;
        const MnoLcTail t{*lc->lp, dRef.dev(), dEn.dev(), dFL.dev(), dIL.dev(), dFR.dev(), dIR.dev(), lrec.dev(), lbest.dev(), lidx.dev(), lcnt.dev(), bidx.dev(), bcnt.dev()};
        rc = enqueue_mno_lc_tail(c, WS.stream, B, K, dSol, t);   // (everything in front of it is complete: the loop above ends on a sync)
        if (rc) return rc;
        rc = m.download();
        if (rc) return rc;
    }
    return scope.close(ROMAN_OK);
}

int roman_mno_batch(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                    const double* feats, int64_t n_objects,
                    const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t F,
                    const int32_t* assoc, const int64_t* assoc_off,
                    int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                    roman_mno_solution_t* sol_out, roman_stats_t* stats_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    return mno_to_host(c, params, B, feats, n_objects, off1, n1, off2, n2, F, assoc, assoc_off, num_solutions, kmax, assoc_out, sol_out, stats_out, nullptr);
}

int roman_mno_lc_batch(roman_ctx_t* c, const roman_params_t* params, int32_t B,
                       const double* feats, int64_t n_objects,
                       const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2, int32_t F,
                       const int32_t* assoc, const int64_t* assoc_off,
                       int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                       roman_mno_solution_t* sol_out, roman_stats_t* stats_out,
                       const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                       const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                       roman_lc_record_t* records, int32_t* best, int32_t* accepted_idx, int32_t* n_accepted,
                       int32_t* accepted_best_idx, int32_t* n_accepted_best)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    MnoLcTail t;
    const int rc = make_mno_lc_tail(c, lc_params, B, num_solutions, T_ref, enable, FL, iL, FR, iR, records, best, accepted_idx, n_accepted, accepted_best_idx, n_accepted_best, &t);
    if (rc) return rc;
    if (params && lc_params->dim != params->point_dim) return fail(c, ROMAN_E_INVALID, "lc_params.dim (%d) differs from params.point_dim (%d)", lc_params->dim, params->point_dim);
    if (n_left < 0 || n_right < 0) return fail(c, ROMAN_E_INVALID, "negative size");
    for (int b = 0; b < B; ++b) {                                // the device indexes the frame pools with these
        if (iL && (iL[b] < 0 || iL[b] >= n_left)) return fail(c, ROMAN_E_INVALID, "iL[%d] = %d outside the %d left frames", b, iL[b], n_left);
        if (iR && (iR[b] < 0 || iR[b] >= n_right)) return fail(c, ROMAN_E_INVALID, "iR[%d] = %d outside the %d right frames", b, iR[b], n_right);
    }
    const MnoLcHost lc{lc_params, T_ref, enable, FL, n_left, iL, FR, n_right, iR, records, best, accepted_idx, n_accepted, accepted_best_idx, n_accepted_best};
    return mno_to_host(c, params, B, feats, n_objects, off1, n1, off2, n2, F, assoc, assoc_off, num_solutions, kmax, assoc_out, sol_out, stats_out, &lc);
}

// --- RANSAC registration on object centres, batched ([REF roman/align/ransac_reg.py:16-53]) ----------------------
static int ransac_check(roman_ctx* c, const roman_ransac_params_t* P, int32_t B, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                        int64_t n_objects /* -1: not known (device pointers) */, int32_t kmax, const void* assoc_out, const void* rec_out)
{
    if (B < 0) return fail(c, ROMAN_E_INVALID, "B < 0");
    if (!P) return fail(c, ROMAN_E_INVALID, "rparams is NULL");
    if (P->max_iteration < 1) return fail(c, ROMAN_E_INVALID, "max_iteration must be >= 1 (got %lld)", (long long)P->max_iteration);
    if (P->round < 1) return fail(c, ROMAN_E_INVALID, "round must be >= 1 (got %d)", P->round);
    if (!(P->edge_len > 0.0 && P->edge_len <= 1.0)) return fail(c, ROMAN_E_INVALID, "edge_len must lie in (0, 1] (got %g)", P->edge_len);
    if (!(P->max_dist > 0.0) || !std::isfinite(P->max_dist)) return fail(c, ROMAN_E_INVALID, "max_dist must be > 0 (got %g)", P->max_dist);
    if (!(P->confidence > 0.0 && P->confidence < 1.0)) return fail(c, ROMAN_E_INVALID, "confidence must lie in (0, 1) (got %g)", P->confidence);
    if (B == 0) return ROMAN_OK;
    if (!rec_out || kmax < 0 || (kmax > 0 && !assoc_out)) return fail(c, ROMAN_E_INVALID, "NULL output pointer or kmax < 0");
    BatchCheck chk; chk.n_objects = n_objects; chk.side_cap = ROMAN_RANSAC_MAX_OBJECTS; chk.cap_code = ROMAN_E_TOO_LARGE; chk.cap_who = "roman_ransac_batch";
    return check_batch(c, B, off1, n1, off2, n2, chk);
}

// k_ransac for B checked problems over rows of F doubles, on the context's stream: descriptors through the pinned staging, one launch
static int enqueue_ransac(roman_ctx* c, const roman_ransac_params_t* rparams, int32_t B, const double* rows, int32_t F,
                          const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                          int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out, const RansacSplit& split)
{
    int maxN = 0; bool any = false;
    for (int b = 0; b < B; ++b) { maxN = std::max(maxN, n1[b] + n2[b]); any = any || (n1[b] > 0 && n2[b] > 0); }
    if (!rows && any) return fail(c, ROMAN_E_INVALID, "pts is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    RansacDesc* staged = nullptr;
    HIPCHK(c, c->ransacStage.stage((size_t)B, &staged));
    for (int b = 0; b < B; ++b) staged[b] = RansacDesc{off1[b], off2[b], n1[b], n2[b]};
    HIPCHK(c, c->ransacStage.upload(c->ransacDesc, (size_t)B, stream));
    const size_t lds = sizeof(double) * 3 * (size_t)std::max(maxN, 1);          // both point sets of the largest problem (at most 48 KB)
    hipLaunchKernelGGL(k_ransac, dim3((unsigned)B), dim3(RANSAC_NT), lds, stream, *rparams, (int)B, c->ransacDesc.as<RansacDesc>(), rows, (int)F,
                       (int)kmax, assoc_out, rec_out, counts_out, split);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_ransac_batch_dev(roman_ctx_t* c, const roman_ransac_params_t* rparams, int32_t B,
                           const double* pts, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                           int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = ransac_check(c, rparams, B, off1, n1, off2, n2, -1, kmax, assoc_out, rec_out);
    if (rc || B == 0) return rc;
    return enqueue_ransac(c, rparams, B, pts, 3, off1, n1, off2, n2, kmax, assoc_out, rec_out, counts_out, RansacSplit{nullptr, nullptr, nullptr});
}

int roman_ransac_batch(roman_ctx_t* c, const roman_ransac_params_t* rparams, int32_t B,
                       const double* pts, int64_t n_objects, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                       int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out)
{
    return roman_ransac_lc_batch(c, rparams, B, pts, n_objects, 3, off1, n1, off2, n2, kmax, assoc_out, rec_out, counts_out, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
}

// --- RANSAC loop closures: k_ransac over strided rows with the tail behind it ([REF roman/align/ransac_reg.py:16-53],
// [REF roman/align/submap_align.py:160-200], [REF roman/align/results.py:156-198]) ---------------------------------
// What both forms check before anything is enqueued, and the tail they enqueue (`t`; used only with lc_params).
static int ransac_lc_check(roman_ctx* c, const roman_ransac_params_t* rparams, int32_t B, int32_t F, const int64_t* off1, const int32_t* n1,
                           const int64_t* off2, const int32_t* n2, int64_t n_objects, int32_t kmax, const void* assoc_out, const void* rec_out,
                           double* T_out, int32_t* n_assoc_out, int32_t* status_out, const roman_lc_params_t* lc_params,
                           const double* T_ref, const int32_t* enable, const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                           roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted, LcTail* t)
{
    int rc = ransac_check(c, rparams, B, off1, n1, off2, n2, n_objects, kmax, assoc_out, rec_out);
    if (rc) return rc;
    if (F < 3) return fail(c, ROMAN_E_INVALID, "F=%d: a row starts with x y z", F);
    if (!lc_params) return ROMAN_OK;
    if (B > 0 && (!T_out || !n_assoc_out || !status_out)) return fail(c, ROMAN_E_INVALID, "the tail reads T_out / n_assoc_out / status_out: NULL split output");
    rc = make_lc_tail(c, lc_params, T_out, n_assoc_out, status_out, T_ref, enable, FL, iL, FR, iR, records, accepted_idx, n_accepted, t);
    if (rc) return rc;
    if (lc_params->dim != 3) return fail(c, ROMAN_E_INVALID, "lc_params.dim must be 3 for RANSAC registration (got %d)", lc_params->dim);
    if (B > 0 && (!records || !accepted_idx)) return fail(c, ROMAN_E_INVALID, "records / accepted_idx is NULL");
    return ROMAN_OK;
}

int roman_ransac_lc_batch_dev(roman_ctx_t* c, const roman_ransac_params_t* rparams, int32_t B,
                              const double* rows, int32_t F, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                              int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out,
                              double* T_out, int32_t* n_assoc_out, int32_t* status_out,
                              const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                              const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                              roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    LcTail t;
    int rc = ransac_lc_check(c, rparams, B, F, off1, n1, off2, n2, -1, kmax, assoc_out, rec_out, T_out, n_assoc_out, status_out, lc_params,
                             T_ref, enable, FL, iL, FR, iR, records, accepted_idx, n_accepted, &t);
    if (rc) return rc;
    if (B > 0) {
        rc = enqueue_ransac(c, rparams, B, rows, F, off1, n1, off2, n2, kmax, assoc_out, rec_out, counts_out, RansacSplit{T_out, n_assoc_out, status_out});
        if (rc) return rc;
    }
    if (!lc_params) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_lc_tail(c, c->stream, B, t);                  // behind k_ransac on the same stream
}

int roman_ransac_lc_batch(roman_ctx_t* c, const roman_ransac_params_t* rparams, int32_t B,
                          const double* rows, int64_t n_objects, int32_t F, const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                          int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out,
                          double* T_out, int32_t* n_assoc_out, int32_t* status_out,
                          const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                          const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                          roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (n_objects < 0) return fail(c, ROMAN_E_INVALID, "negative size");
    LcTail t;
    int rc = ransac_lc_check(c, rparams, B, F, off1, n1, off2, n2, n_objects, kmax, assoc_out, rec_out, T_out, n_assoc_out, status_out, lc_params,
                             T_ref, enable, FL, iL, FR, iR, records, accepted_idx, n_accepted, &t);
    if (rc) return rc;
    if (lc_params) {
        if (n_left < 0 || n_right < 0) return fail(c, ROMAN_E_INVALID, "negative size");
        for (int b = 0; b < B; ++b) {                            // the device indexes the frame pools with these
            if (iL && (iL[b] < 0 || iL[b] >= n_left)) return fail(c, ROMAN_E_INVALID, "iL[%d] = %d outside the %d left frames", b, iL[b], n_left);
            if (iR && (iR[b] < 0 || iR[b] >= n_right)) return fail(c, ROMAN_E_INVALID, "iR[%d] = %d outside the %d right frames", b, iR[b], n_right);
        }
    }
    if (B == 0) { if (lc_params) *n_accepted = 0; return ROMAN_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    c->last.scored = false; c->last.solved = false;            // workspace 0's feature staging is reused: the stepwise problem it held is gone
    const double* dRows = nullptr;
    rc = upload_inputs(c, rows, n_objects, F, 0, nullptr, 0, &dRows);
    if (rc) return rc;
    const size_t nb = (size_t)B, rowsPer = (size_t)kmax * 2, nCounts = counts_out ? nb * (size_t)rparams->max_iteration : 0;
    HostMirror m(c);
    const auto rec = m.out(rec_out, sizeof(roman_ransac_record_t) * nb);
    const auto arows = m.out(assoc_out, sizeof(int32_t) * nb * rowsPer);
    const auto cnt = m.inout(counts_out, sizeof(int32_t) * nCounts);            // entries beyond n_hyp come back as they were
    const auto sT = m.out(T_out, T_out ? sizeof(double) * 16 * nb : 0);
    const auto sN = m.out(n_assoc_out, n_assoc_out ? sizeof(int32_t) * nb : 0);
    const auto sS = m.out(status_out, status_out ? sizeof(int32_t) * nb : 0);
    const bool lc = lc_params != nullptr;
    const auto dRef = m.in(T_ref, lc && T_ref ? sizeof(double) * 16 * nb : 0);
    const auto dEn = m.in(enable, lc && enable ? sizeof(int32_t) * nb : 0);
    const auto dFL = m.in(FL, lc && FL ? sizeof(double) * 16 * (size_t)n_left : 0);
    const auto dIL = m.in(iL, lc && iL ? sizeof(int32_t) * nb : 0);
    const auto dFR = m.in(FR, lc && FR ? sizeof(double) * 16 * (size_t)n_right : 0);
    const auto dIR = m.in(iR, lc && iR ? sizeof(int32_t) * nb : 0);
    const auto lrec = m.out(records, lc ? sizeof(roman_lc_record_t) * nb : 0);
    const auto lidx = m.out(accepted_idx, lc ? sizeof(int32_t) * nb : 0);
    const auto lcnt = m.out(n_accepted, lc ? sizeof(int32_t) : 0);
    rc = m.upload();
    if (rc) return rc;
    const int chunk = std::max(1, c->host_chunk);
    for (int lo = 0; lo < B; lo += chunk) {
        const int hi = std::min(B, lo + chunk);
        const RansacSplit split{sT.dev() ? sT.dev() + (size_t)lo * 16 : nullptr, sN.dev() ? sN.dev() + lo : nullptr, sS.dev() ? sS.dev() + lo : nullptr};
        rc = enqueue_ransac(c, rparams, hi - lo, dRows, F, off1 + lo, n1 + lo, off2 + lo, n2 + lo, kmax, arows.dev() ? arows.dev() + (size_t)lo * rowsPer : nullptr,
                            rec.dev() + lo, nCounts ? cnt.dev() + (size_t)lo * (size_t)rparams->max_iteration : nullptr, split);
        if (rc) return rc;
    }
    if (lc) {                                                    // the tail ONCE over the whole batch, behind the last chunk
        t.in = LcIn{sT.dev(), sN.dev(), sS.dev(), dRef.dev(), dEn.dev(), dFL.dev(), dIL.dev(), dFR.dev(), dIR.dev()};
        t.rec = lrec.dev(); t.idx = lidx.dev(); t.cnt = lcnt.dev();
        rc = enqueue_lc_tail(c, WS.stream, B, t);
        if (rc) return rc;
    }
    return m.download();
}

// --- submaps from a whole map, radius mode ([REF roman/map/map.py:297-346]) ---------------------------------------
static int submaps_check(roman_ctx* c, const roman_submap_params_t* P, int32_t N, int32_t F, const void* seg_feats, const void* seg_times, const void* seg_ids,
                         int32_t S, const void* descs, const void* pool, const void* count, const void* src, const void* ids_out, const void* status,
                         int32_t desc_dim, const void* desc_out, bool pool_needed)
{
    if (!P) return fail(c, ROMAN_E_INVALID, "sparams is NULL");
    if (P->point_dim != 2 && P->point_dim != 3) return fail(c, ROMAN_E_INVALID, "point_dim must be 2 or 3 (got %d)", P->point_dim);
    if (N < 0 || S < 0) return fail(c, ROMAN_E_INVALID, "N < 0 or S < 0");
    if (F < 3) return fail(c, ROMAN_E_INVALID, "F=%d: a segment row starts with x y z", F);
    if (P->cap < 1) return fail(c, ROMAN_E_INVALID, "cap must be >= 1 (got %d)", P->cap);
    if (P->max_size > 0 && P->cap != P->max_size) return fail(c, ROMAN_E_INVALID, "cap (%d) must equal max_size (%d) when max_size is set", P->cap, P->max_size);
    if (P->reserved0 != 0 || P->reserved[0] != 0 || P->reserved[1] != 0) return fail(c, ROMAN_E_INVALID, "roman_submap_params_t reserved words must be 0");
    if (P->use_radius && P->radius != P->radius) return fail(c, ROMAN_E_INVALID, "radius is NaN");
    if (desc_dim < 0 || desc_dim > F - 3) return fail(c, ROMAN_E_INVALID, "desc_dim=%d outside [0, F - 3]", desc_dim);
    if (desc_out && desc_dim == 0) return fail(c, ROMAN_E_INVALID, "desc_out given with desc_dim 0");
    if (ids_out && !seg_ids) return fail(c, ROMAN_E_INVALID, "ids_out given without seg_ids");
    if (S == 0) return ROMAN_OK;
    if (!descs || !count || !src || !status || (pool_needed && !pool)) return fail(c, ROMAN_E_INVALID, "NULL descriptor or output pointer");
    if (N > 0 && (!seg_feats || !seg_times)) return fail(c, ROMAN_E_INVALID, "seg_feats / seg_times is NULL");
    return ROMAN_OK;
}

// --- the submaps of every map of a session in one launch sequence -------------------------------------------------
// What one call of ANY form works on, under names, from the C entry point to the launch: a single map is a session of one map (its two
// offset tables on the entry point's stack).  The host forms hand the launch a copy whose bulk arrays are the mirror's; seg_off,
// sub_off, descs and list are HOST memory in every form.  What tells the forms apart is data:
//   listed  only the L submaps of `list` are rebuilt, whole, in place; `changed` (or NULL) learns which slots differ
//   fill    count and src are the CALLER's lists: nothing is selected, seg_times and status are not read
struct SubmapsArgs {
    int32_t R, F;
    const int64_t* seg_off; const double* seg_feats; const double* seg_times; const int64_t* seg_ids;
    const int32_t* sub_off; const roman_submap_desc_t* descs;
    double* pool; int32_t* count; int32_t* src; int64_t* ids_out; int32_t* status;
    int32_t desc_dim; double* desc_out;
    bool listed; int32_t L; const int32_t* list; int32_t* changed;
    bool fill;
};

// The checks of the session entry points, on host memory only, a NULL context included (fail() then keeps the text for
// roman_last_error(NULL)): the offsets first (they size everything else), then roman_submaps_dev's own checks, the list (DESIGN.md
// §4.21) behind them, the context last.  What passes has *n submaps to launch; 0: the call is empty.
static int session_submaps_check(roman_ctx* c, const roman_submap_params_t* P, const SubmapsArgs& g, bool pool_needed, int32_t* n)
{
    const int32_t R = g.R;
    if (R < 0) return fail(c, ROMAN_E_INVALID, "R < 0");
    if (R > 0 && (!g.seg_off || !g.sub_off)) return fail(c, ROMAN_E_INVALID, "seg_off / sub_off is NULL");
    if (R > 0 && (g.seg_off[0] != 0 || g.sub_off[0] != 0)) return fail(c, ROMAN_E_INVALID, "seg_off[0] and sub_off[0] must be 0");
    for (int r = 0; r < R; ++r) {
        if (g.seg_off[r + 1] < g.seg_off[r]) return fail(c, ROMAN_E_INVALID, "seg_off decreases at map %d", r);
        if (g.sub_off[r + 1] < g.sub_off[r]) return fail(c, ROMAN_E_INVALID, "sub_off decreases at map %d", r);
        if (g.seg_off[r + 1] - g.seg_off[r] > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "map %d holds more than %d segments", r, INT32_MAX);
    }
    const int64_t N = R > 0 ? g.seg_off[R] : 0;
    const int32_t S = R > 0 ? g.sub_off[R] : 0;
    int rc = submaps_check(c, P, N > 0 ? 1 : 0, g.F, g.seg_feats, g.seg_times, g.seg_ids, S, g.descs, g.pool, g.count, g.src, g.ids_out, g.status,
                           g.desc_dim, g.desc_out, pool_needed);
    if (rc) return rc;
    if ((int64_t)S * P->cap > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "sub_off[R] * cap = %lld rows exceed the index width", (long long)S * P->cap);
    if (g.listed) {
        if (g.L < 0) return fail(c, ROMAN_E_INVALID, "L < 0");
        if (g.L > 0 && !g.list) return fail(c, ROMAN_E_INVALID, "list is NULL");
        for (int32_t l = 0; l < g.L; ++l) {
            if (g.list[l] < 0 || g.list[l] >= S) return fail(c, ROMAN_E_INVALID, "list[%d] = %d outside the %d submaps of the session", l, g.list[l], S);
            if (l > 0 && g.list[l] <= g.list[l - 1]) return fail(c, ROMAN_E_INVALID, "list is not strictly ascending at entry %d", l);
        }
    }
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    *n = g.listed ? g.L : S;
    return ROMAN_OK;
}

// --- force-fill submaps and the boxes of a pool ([REF roman/map/map.py:264-295], [REF :133-139]) -------------------
static int submaps_fill_check(roman_ctx* c, int32_t point_dim, int32_t cap, int32_t N, int32_t F, const void* seg_feats, const void* seg_ids,
                              int32_t S, const void* descs, const void* count, const void* src, const void* pool, const void* ids_out,
                              int32_t desc_dim, const void* desc_out, bool pool_needed)
{
    if (point_dim != 2 && point_dim != 3) return fail(c, ROMAN_E_INVALID, "point_dim must be 2 or 3 (got %d)", point_dim);
    if (N < 0 || S < 0) return fail(c, ROMAN_E_INVALID, "N < 0 or S < 0");
    if (F < 3) return fail(c, ROMAN_E_INVALID, "F=%d: a segment row starts with x y z", F);
    if (cap < 1) return fail(c, ROMAN_E_INVALID, "cap must be >= 1 (got %d)", cap);
    if (desc_dim < 0 || desc_dim > F - 3) return fail(c, ROMAN_E_INVALID, "desc_dim=%d outside [0, F - 3]", desc_dim);
    if (desc_out && desc_dim == 0) return fail(c, ROMAN_E_INVALID, "desc_out given with desc_dim 0");
    if (ids_out && !seg_ids) return fail(c, ROMAN_E_INVALID, "ids_out given without seg_ids");
    if (S == 0) return ROMAN_OK;
    if (!descs || !count || !src || (pool_needed && !pool)) return fail(c, ROMAN_E_INVALID, "NULL descriptor, count, src or pool pointer");
    if (N > 0 && !seg_feats) return fail(c, ROMAN_E_INVALID, "seg_feats is NULL");
    return ROMAN_OK;
}

// --- one path under every form: the job table, the launches, the host-pointer mirror --------------------------------------------------
// The staged job table of one call: its device copy, the staging it went up from, its records, the largest map that has one.
struct SubmapJobs { const SubmapJob* dev; const SubmapJob* host; int32_t n, maxN; };

// One record per LAUNCHED submap — all sub_off[R] of them, or the L of `list` (strictly ascending) —, each with its map's rows and its
// slice of the spill, which starts where the slices of the launched submaps in front of it end (`select`: the call selects, so it needs
// the spill and the dense centres at all).  Every scratch is had before the table goes up: a failure leaves nothing enqueued.
static int submaps_stage(roman_ctx* c, int32_t R, const int64_t* seg_off, const int32_t* sub_off, const roman_submap_desc_t* descs,
                         int32_t L, const int32_t* list, bool select, SubmapJobs* out)
{
    const int32_t n = list ? L : sub_off[R];
    SubmapJob* jobs = nullptr;
    HIPCHK(c, c->smStage.stage((size_t)n, &jobs));
    int64_t spill = 0; int32_t maxN = 0;
    for (int32_t r = 0, j = 0; r < R && j < n; ++r) {
        const int64_t rows = seg_off[r + 1] - seg_off[r], over = select ? std::max<int64_t>(rows - SUBMAP_LDS_CAND, 0) : 0;
        int32_t j1 = j;                                          // the launched submaps of map r: jobs [j, j1)
        if (!list) j1 = sub_off[r + 1]; else while (j1 < n && list[j1] < sub_off[r + 1]) ++j1;
        if (j1 == j) continue;
        maxN = std::max(maxN, (int32_t)rows);
        if (over && j1 - j > (INT64_MAX / 16 - spill) / over)
            return fail(c, ROMAN_E_NOMEM, "the candidate scratch of the %s exceeds the address space", list ? "listed submaps" : "session");
        for (; j < j1; ++j, spill += over) {
            const int32_t g = list ? list[j] : j;
            jobs[j] = SubmapJob{descs[g], seg_off[r], spill, (int32_t)rows, g};
        }
    }
    if (spill > 0) {
        HIPCHK(c, c->smSpillKey.ensure(sizeof(double) * (size_t)spill));
        HIPCHK(c, c->smSpillIdx.ensure(sizeof(int32_t) * (size_t)spill));
    }
    if (select) HIPCHK(c, c->smPts.ensure(sizeof(double) * 3 * (size_t)std::max<int64_t>(seg_off[R], 1)));
    HIPCHK(c, c->smStage.upload(c->smJobs, (size_t)n, c->stream));
    *out = SubmapJobs{c->smJobs.as<SubmapJob>(), jobs, n, maxN};
    return ROMAN_OK;
}

// The device-pointer call of every form, behind its entry point's checks: there is a submap to launch.
static int submaps_launch(roman_ctx* c, const roman_submap_params_t* P, const SubmapsArgs& g)
{
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    const int cap = P->cap, F = g.F, d = g.desc_dim;
    const auto feats = reinterpret_cast<const unsigned long long*>(g.seg_feats);
    if (g.listed) HIPCHK(c, c->smListOut.ensure(sizeof(int32_t) * ((size_t)g.L * (size_t)cap + 2 * (size_t)g.L)));
    SubmapJobs J;
    int rc = submaps_stage(c, g.R, g.seg_off, g.sub_off, g.descs, g.L, g.listed ? g.list : nullptr, !g.fill, &J);
    if (rc) return rc;
    // what the select writes: the caller's arrays, or — the list form, whose store kernel compares before it writes — the context's scratch
    int32_t* src = g.listed ? c->smListOut.as<int32_t>() : g.src;
    int32_t* count = g.listed ? src + (size_t)J.n * (size_t)cap : g.count;
    int32_t* status = g.listed ? count + J.n : g.status;
    if (!g.fill) {
        // the dense centres: of the whole session at once, or — the list form — of the maps that have a listed submap, each map's rows
        // at their place in the session's array (the records of one map lie together; maps without rows launch nothing)
        double* pts = c->smPts.as<double>();
        const int64_t N = g.seg_off[g.R];
        if (!g.listed && N > 0) hipLaunchKernelGGL(k_submap_points, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, F, g.seg_feats, pts);
        for (int32_t l = 0; g.listed && l < J.n; ++l) {
            const SubmapJob& a = J.host[l];
            if (a.N > 0 && (l == 0 || J.host[l - 1].seg0 != a.seg0 || J.host[l - 1].N != a.N))
                hipLaunchKernelGGL(k_submap_points, dim3((unsigned)(((int64_t)a.N + 255) / 256)), dim3(256), 0, stream, (int64_t)a.N, F,
                                   g.seg_feats + a.seg0 * F, pts + 3 * a.seg0);
        }
        hipLaunchKernelGGL(k_submap_select, dim3((unsigned)J.n), dim3(SUBMAP_NT), 0, stream, *P, (int)J.n, J.dev, pts, g.seg_times,
                           c->smSpillKey.as<double>(), c->smSpillIdx.as<int32_t>(), count, src, status);
        HIPCHK(c, hipGetLastError());
    }
    if (g.listed) {
        const auto store = g.changed ? k_submap_store_list<true> : k_submap_store_list<false>;
        hipLaunchKernelGGL(store, dim3((unsigned)J.n), dim3(256), 0, stream, (int)P->point_dim, cap, F, d, J.dev, feats, g.seg_ids, count, src, status,
                           reinterpret_cast<unsigned long long*>(g.pool), g.count, g.src, g.ids_out, g.status, reinterpret_cast<unsigned long long*>(g.desc_out),
                           g.changed);
    } else if (J.maxN > 0) {
        // a wave per row, four rows per workgroup and pass: enough row groups for the largest slot of the largest map, at most 64 per submap
        const unsigned groups = (unsigned)std::min(64, (std::min(cap, J.maxN) + 3) / 4);
        hipLaunchKernelGGL(k_submap_gather, dim3((unsigned)J.n, groups), dim3(256), 0, stream, (int)P->point_dim, cap, F, J.dev, feats, g.seg_ids, count, src,
                           reinterpret_cast<unsigned long long*>(g.pool), g.ids_out);
        if (g.desc_out) hipLaunchKernelGGL(k_submap_desc, dim3((unsigned)J.n, (unsigned)((d + 255) / 256)), dim3(256), 0, stream, cap, F, d, J.dev, g.seg_feats,
                                           count, src, g.desc_out);
    }
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// The host-pointer call of every form: the bulk arrays as one block of the mirror, submaps_launch() on it, the outputs back.  The
// caller's src, ids_out, desc_out and pool go up first: what the launch leaves untouched comes back as it was, and without a pool the
// launch still writes one.  count and status are written whole — but the list form changes the listed slots only (and `changed`
// compares with what was there), and a fill call only reads the caller's count and src.
static int submaps_mirror(roman_ctx* c, const roman_submap_params_t* P, const SubmapsArgs& h)
{
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const size_t N = (size_t)h.seg_off[h.R], S = (size_t)h.sub_off[h.R];
    const size_t rows = S * (size_t)P->cap, bPool = sizeof(double) * rows * (size_t)(P->point_dim + h.F - 3);
    const unsigned lists = h.fill ? HostMirror::UP : HostMirror::UP | HostMirror::DOWN;
    const unsigned words = h.fill ? HostMirror::UP : h.listed ? HostMirror::UP | HostMirror::DOWN : HostMirror::DOWN;
    HostMirror m(c);
    const auto feats = m.in(h.seg_feats, sizeof(double) * N * (size_t)h.F);
    const auto times = m.in(h.seg_times, h.fill ? 0 : sizeof(double) * 2 * N);
    const auto ids = m.in(h.seg_ids, h.seg_ids ? sizeof(int64_t) * N : 0);
    const auto dPool = h.pool ? m.inout(h.pool, bPool) : m.room<double>(bPool);
    const auto idsOut = m.inout(h.ids_out, h.ids_out ? sizeof(int64_t) * rows : 0);
    const auto descOut = m.inout(h.desc_out, h.desc_out ? sizeof(double) * S * (size_t)h.desc_dim : 0);
    const auto dSrc = m.piece(h.src, sizeof(int32_t) * rows, lists);
    const auto cnt = m.piece(h.count, sizeof(int32_t) * S, words);
    const auto st = m.piece(h.status, h.status ? sizeof(int32_t) * S : 0, words);
    const auto chg = m.out(h.changed, h.changed ? sizeof(int32_t) * (size_t)h.L : 0);
    int rc = m.upload();
    if (rc) return rc;
    SubmapsArgs g = h;                                           // the same call on the mirror; offsets, descriptors and list stay the caller's
    g.seg_feats = feats.dev(); g.seg_times = times.dev(); g.seg_ids = ids.dev();
    g.pool = dPool.dev(); g.count = cnt.dev(); g.src = dSrc.dev(); g.ids_out = idsOut.dev(); g.status = st.dev(); g.desc_out = descOut.dev();
    g.changed = chg.dev();
    rc = submaps_launch(c, P, g);
    if (rc) return rc;
    return m.download();
}

// --- the entry points: each its own checks, then the argument block and the one path ------------------------------------------------
int roman_submaps_dev(roman_ctx_t* c, const roman_submap_params_t* sparams, int32_t N, int32_t F,
                      const double* seg_feats, const double* seg_times, const int64_t* seg_ids, int32_t S, const roman_submap_desc_t* descs,
                      double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status, int32_t desc_dim, double* desc_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = submaps_check(c, sparams, N, F, seg_feats, seg_times, seg_ids, S, descs, pool, count, src, ids_out, status, desc_dim, desc_out, true);
    if (rc || S == 0) return rc;
    const int64_t seg_off[2] = {0, N}; const int32_t sub_off[2] = {0, S};
    const SubmapsArgs g{1, F, seg_off, seg_feats, seg_times, seg_ids, sub_off, descs, pool, count, src, ids_out, status, desc_dim, desc_out};
    return submaps_launch(c, sparams, g);
}

int roman_submaps(roman_ctx_t* c, const roman_submap_params_t* sparams, int32_t N, int32_t F,
                  const double* seg_feats, const double* seg_times, const int64_t* seg_ids, int32_t S, const roman_submap_desc_t* descs,
                  double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status, int32_t desc_dim, double* desc_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = submaps_check(c, sparams, N, F, seg_feats, seg_times, seg_ids, S, descs, pool, count, src, ids_out, status, desc_dim, desc_out, false);
    if (rc || S == 0) return rc;
    const int64_t seg_off[2] = {0, N}; const int32_t sub_off[2] = {0, S};
    const SubmapsArgs h{1, F, seg_off, seg_feats, seg_times, seg_ids, sub_off, descs, pool, count, src, ids_out, status, desc_dim, desc_out};
    return submaps_mirror(c, sparams, h);
}

int roman_session_submaps_dev(roman_ctx_t* c, const roman_submap_params_t* sparams, int32_t R, int32_t F, const int64_t* seg_off,
                              const double* seg_feats, const double* seg_times, const int64_t* seg_ids, const int32_t* sub_off, const roman_submap_desc_t* descs,
                              double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status, int32_t desc_dim, double* desc_out)
{
    const SubmapsArgs g{R, F, seg_off, seg_feats, seg_times, seg_ids, sub_off, descs, pool, count, src, ids_out, status, desc_dim, desc_out};
    int32_t n = 0;
    const int rc = session_submaps_check(c, sparams, g, true, &n);
    return rc || n == 0 ? rc : submaps_launch(c, sparams, g);
}

int roman_session_submaps(roman_ctx_t* c, const roman_submap_params_t* sparams, int32_t R, int32_t F, const int64_t* seg_off,
                          const double* seg_feats, const double* seg_times, const int64_t* seg_ids, const int32_t* sub_off, const roman_submap_desc_t* descs,
                          double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status, int32_t desc_dim, double* desc_out)
{
    const SubmapsArgs h{R, F, seg_off, seg_feats, seg_times, seg_ids, sub_off, descs, pool, count, src, ids_out, status, desc_dim, desc_out};
    int32_t n = 0;
    const int rc = session_submaps_check(c, sparams, h, false, &n);
    return rc || n == 0 ? rc : submaps_mirror(c, sparams, h);
}

int roman_session_submaps_list_dev(roman_ctx_t* c, const roman_submap_params_t* sparams, int32_t R, int32_t F, const int64_t* seg_off,
                                   const double* seg_feats, const double* seg_times, const int64_t* seg_ids, const int32_t* sub_off, const roman_submap_desc_t* descs,
                                   double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status, int32_t desc_dim, double* desc_out,
                                   int32_t L, const int32_t* list, int32_t* changed)
{
    const SubmapsArgs g{R, F, seg_off, seg_feats, seg_times, seg_ids, sub_off, descs, pool, count, src, ids_out, status, desc_dim, desc_out,
                        true, L, list, changed};
    int32_t n = 0;
    const int rc = session_submaps_check(c, sparams, g, true, &n);
    return rc || n == 0 ? rc : submaps_launch(c, sparams, g);
}

int roman_session_submaps_list(roman_ctx_t* c, const roman_submap_params_t* sparams, int32_t R, int32_t F, const int64_t* seg_off,
                               const double* seg_feats, const double* seg_times, const int64_t* seg_ids, const int32_t* sub_off, const roman_submap_desc_t* descs,
                               double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status, int32_t desc_dim, double* desc_out,
                               int32_t L, const int32_t* list, int32_t* changed)
{
    const SubmapsArgs h{R, F, seg_off, seg_feats, seg_times, seg_ids, sub_off, descs, pool, count, src, ids_out, status, desc_dim, desc_out,
                        true, L, list, changed};
    int32_t n = 0;
    const int rc = session_submaps_check(c, sparams, h, true, &n);
    return rc || n == 0 ? rc : submaps_mirror(c, sparams, h);
}

// The fill forms' argument block: the caller's lists stand where the select's outputs do (nothing writes them), and of the parameters
// only point_dim and cap exist.
static SubmapsArgs submaps_fill_args(roman_submap_params_t* P, int32_t point_dim, int32_t cap, int32_t F, const int64_t* seg_off, const double* seg_feats,
                                     const int64_t* seg_ids, const int32_t* sub_off, const roman_submap_desc_t* descs, const int32_t* count,
                                     const int32_t* src, double* pool, int64_t* ids_out, int32_t desc_dim, double* desc_out)
{
    *P = roman_submap_params_t{};
    P->point_dim = point_dim; P->cap = cap;
    SubmapsArgs g{1, F, seg_off, seg_feats, nullptr, seg_ids, sub_off, descs, pool, const_cast<int32_t*>(count), const_cast<int32_t*>(src), ids_out, nullptr,
                  desc_dim, desc_out};
    g.fill = true;
    return g;
}

int roman_submaps_fill_dev(roman_ctx_t* c, int32_t point_dim, int32_t cap, int32_t N, int32_t F,
                           const double* seg_feats, const int64_t* seg_ids, int32_t S, const roman_submap_desc_t* descs,
                           const int32_t* count, const int32_t* src, double* pool, int64_t* ids_out, int32_t desc_dim, double* desc_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = submaps_fill_check(c, point_dim, cap, N, F, seg_feats, seg_ids, S, descs, count, src, pool, ids_out, desc_dim, desc_out, true);
    if (rc || S == 0 || N == 0) return rc;
    const int64_t seg_off[2] = {0, N}; const int32_t sub_off[2] = {0, S};
    roman_submap_params_t P;
    const SubmapsArgs g = submaps_fill_args(&P, point_dim, cap, F, seg_off, seg_feats, seg_ids, sub_off, descs, count, src, pool, ids_out, desc_dim, desc_out);
    return submaps_launch(c, &P, g);
}

int roman_submaps_fill(roman_ctx_t* c, int32_t point_dim, int32_t cap, int32_t N, int32_t F,
                       const double* seg_feats, const int64_t* seg_ids, int32_t S, const roman_submap_desc_t* descs,
                       const int32_t* count, const int32_t* src, double* pool, int64_t* ids_out, int32_t desc_dim, double* desc_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = submaps_fill_check(c, point_dim, cap, N, F, seg_feats, seg_ids, S, descs, count, src, pool, ids_out, desc_dim, desc_out, false);
    if (rc || S == 0) return rc;
    // the host holds the lists: every row a map index, every count inside its slot
    for (int32_t s = 0; s < S; ++s) {
        if (count[s] < 0 || count[s] > cap) return fail(c, ROMAN_E_INVALID, "count[%d]=%d outside [0, cap]", s, count[s]);
        for (int32_t r = 0; r < count[s]; ++r) {
            const int32_t k = src[(size_t)s * (size_t)cap + (size_t)r];
            if (k < 0 || k >= N) return fail(c, ROMAN_E_INVALID, "src[%d][%d]=%d is not a map index", s, r, k);
        }
    }
    if (N == 0) return ROMAN_OK;
    const int64_t seg_off[2] = {0, N}; const int32_t sub_off[2] = {0, S};
    roman_submap_params_t P;
    const SubmapsArgs h = submaps_fill_args(&P, point_dim, cap, F, seg_off, seg_feats, seg_ids, sub_off, descs, count, src, pool, ids_out, desc_dim, desc_out);
    return submaps_mirror(c, &P, h);
}

static int submap_boxes_check(roman_ctx* c, int32_t S, int32_t F, int32_t cap, const void* pool, const void* count, const void* T_odom_center, const void* box)
{
    if (S < 0) return fail(c, ROMAN_E_INVALID, "S < 0");
    if (F < 3) return fail(c, ROMAN_E_INVALID, "F=%d: a pool row starts with x y z", F);
    if (cap < 1) return fail(c, ROMAN_E_INVALID, "cap must be >= 1 (got %d)", cap);
    if (S == 0) return ROMAN_OK;
    if (!pool || !count || !T_odom_center || !box) return fail(c, ROMAN_E_INVALID, "NULL pool, count, T_odom_center or box pointer");
    return ROMAN_OK;
}

int roman_submap_boxes_dev(roman_ctx_t* c, int32_t S, int32_t F, int32_t cap, const double* pool, const int32_t* count,
                           const double* T_odom_center, double* box)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = submap_boxes_check(c, S, F, cap, pool, count, T_odom_center, box);
    if (rc || S == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_submap_boxes, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, c->stream, (int)S, (int)F, (int)cap, pool, count, T_odom_center, box);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_submap_boxes(roman_ctx_t* c, int32_t S, int32_t F, int32_t cap, const double* pool, const int32_t* count,
                       const double* T_odom_center, double* box)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = submap_boxes_check(c, S, F, cap, pool, count, T_odom_center, box);
    if (rc || S == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HostMirror m(c);
    const auto dPool = m.in(pool, sizeof(double) * (size_t)S * (size_t)cap * (size_t)F);
    const auto cnt = m.in(count, sizeof(int32_t) * (size_t)S);
    const auto T = m.in(T_odom_center, sizeof(double) * 16 * (size_t)S);
    const auto dBox = m.out(box, sizeof(double) * 6 * (size_t)S);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_submap_boxes_dev(c, S, F, cap, dPool.dev(), cnt.dev(), T.dev(), dBox.dev());
    if (rc) return rc;
    return m.download();
}

// --- the boxes of every submap of a session over the concatenated pools ------------------------------------------
static int session_boxes_check(roman_ctx* c, int32_t S, int32_t F, const void* pool, const void* row0, const void* count, const void* T_odom_center, const void* box)
{
    if (S < 0) return fail(c, ROMAN_E_INVALID, "S < 0");
    if (F < 3) return fail(c, ROMAN_E_INVALID, "F=%d: a pool row starts with x y z", F);
    if (S == 0) return ROMAN_OK;
    if (!pool || !row0 || !count || !T_odom_center || !box) return fail(c, ROMAN_E_INVALID, "NULL pool, row0, count, T_odom_center or box pointer");
    return ROMAN_OK;
}

int roman_session_boxes_dev(roman_ctx_t* c, int32_t S, int32_t F, const double* pool, const int64_t* row0, const int32_t* count,
                            const double* T_odom_center, double* box)
{
    int rc = session_boxes_check(c, S, F, pool, row0, count, T_odom_center, box);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (S == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_session_boxes, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, c->stream, (int)S, (int)F, pool, row0, count, T_odom_center, box);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_session_boxes(roman_ctx_t* c, int32_t S, int32_t F, const double* pool, const int64_t* row0, const int32_t* count,
                        const double* T_odom_center, double* box)
{
    int rc = session_boxes_check(c, S, F, pool, row0, count, T_odom_center, box);
    if (rc) return rc;
    int64_t rows = 0;                                            // the rows of `pool` the submaps name: what goes up
    for (int g = 0; g < S; ++g) {
        if (count[g] < 0 || row0[g] < 0) return fail(c, ROMAN_E_INVALID, "submap %d: row0=%lld, count=%d must not be negative", g, (long long)row0[g], count[g]);
        if (count[g] > 0) rows = std::max(rows, row0[g] + (int64_t)count[g]);
    }
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (S == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HostMirror m(c);
    const auto dPool = m.in(pool, sizeof(double) * (size_t)rows * (size_t)F);
    const auto dRow = m.in(row0, sizeof(int64_t) * (size_t)S);
    const auto cnt = m.in(count, sizeof(int32_t) * (size_t)S);
    const auto T = m.in(T_odom_center, sizeof(double) * 16 * (size_t)S);
    const auto dBox = m.out(box, sizeof(double) * 6 * (size_t)S);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_session_boxes_dev(c, S, F, rows ? dPool.dev() : reinterpret_cast<const double*>(dRow.dev()) /* never read: every count is 0 */, dRow.dev(), cnt.dev(),
                                 T.dev(), dBox.dev());
    if (rc) return rc;
    return m.download();
}

// --- segment tables from point clouds ------------------------------------------------------------------------------
static_assert(SEG_BLOCK_MIN == ROMAN_SEG_BLOCK_MIN && SEG_ST_EMPTY == ROMAN_SEG_EMPTY && SEG_ST_FEW_POINTS == ROMAN_SEG_FEW_POINTS &&
              SEG_ST_DEGENERATE == ROMAN_SEG_DEGENERATE, "kernels.hip.h and roman_hip.h name the same numbers");
static_assert(sizeof(roman_segment_shape_params_t) == 32, "roman_segment_shape_params_t is eight int32 words");

// the offsets of N point clouds stored one behind the other (seg_off of roman_segment_shapes*, cloud_off of roman_assoc_scores*)
static int cloud_offsets_check(roman_ctx* c, const int64_t* off, int64_t N, const char* name, const char* item)
{
    if (off[0] != 0) return fail(c, ROMAN_E_INVALID, "%s[0] = %lld: the first %s starts at row 0", name, (long long)off[0], item);
    for (int64_t i = 0; i < N; ++i) {
        if (off[i + 1] < off[i]) return fail(c, ROMAN_E_INVALID, "%s descends at %s %lld", name, item, (long long)i);
        if (off[i + 1] - off[i] > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "%s %lld holds more than %d points", item, (long long)i, INT32_MAX);
    }
    return ROMAN_OK;
}

// everything roman_segment_shapes* judge on host memory -> *P_out: the rows of `points`
static int segment_shapes_check(roman_ctx* c, const void* points, const int64_t* seg_off, int32_t N, const roman_segment_shape_params_t* P,
                                const void* out, const void* status, int64_t* P_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (!P) return fail(c, ROMAN_E_INVALID, "params is NULL");
    if (!seg_off) return fail(c, ROMAN_E_INVALID, "seg_off is NULL");
    if (N < 0) return fail(c, ROMAN_E_INVALID, "N < 0");
    { const int rc = cloud_offsets_check(c, seg_off, N, "seg_off", "segment"); if (rc) return rc; }
    if (P->center_ref != ROMAN_CENTER_MEAN && P->center_ref != ROMAN_CENTER_BOTTOM_MIDDLE) return fail(c, ROMAN_E_INVALID, "unknown center_ref %d", P->center_ref);
    if (P->out_stride < 1) return fail(c, ROMAN_E_INVALID, "out_stride must be >= 1 (got %d)", P->out_stride);
    if (P->col_center < 0) return fail(c, ROMAN_E_INVALID, "col_center = %d: the centre is always written", P->col_center);
    if (P->col_pca < -1 || P->col_volume < -1 || P->col_extent < -1) return fail(c, ROMAN_E_INVALID, "a column is < -1 (-1: not written)");
    const int32_t col[4] = {P->col_center, P->col_pca, P->col_volume, P->col_extent}, width[4] = {3, 3, 1, 3};
    for (int a = 0; a < 4; ++a) {
        if (col[a] < 0) continue;
        if ((int64_t)col[a] + width[a] > (int64_t)P->out_stride) return fail(c, ROMAN_E_INVALID, "columns %d..%d leave out_stride = %d", col[a], col[a] + width[a] - 1, P->out_stride);
        for (int b = 0; b < a; ++b)
            if (col[b] >= 0 && col[a] < col[b] + width[b] && col[b] < col[a] + width[a])
                return fail(c, ROMAN_E_INVALID, "the written columns from %d and from %d overlap", col[b], col[a]);
    }
    if (P->reserved[0] || P->reserved[1]) return fail(c, ROMAN_E_INVALID, "reserved words of roman_segment_shape_params_t must be 0");
    *P_out = seg_off[N];
    if (*P_out > 0 && !points) return fail(c, ROMAN_E_INVALID, "points is NULL");
    if (N > 0 && (!out || !status)) return fail(c, ROMAN_E_INVALID, "out / status is NULL");
    return ROMAN_OK;
}

int roman_segment_shapes_dev(roman_ctx_t* c, const double* points, const int64_t* seg_off_dev, const int64_t* seg_off_host, int32_t N,
                             const roman_segment_shape_params_t* params, double* out, int32_t* status)
{
    int64_t P = 0;
    int rc = segment_shapes_check(c, points, seg_off_host, N, params, out, status, &P);
    if (rc) return rc;
    if (N > 0 && !seg_off_dev) return fail(c, ROMAN_E_INVALID, "seg_off is NULL on the device");
    if (N == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // ---- the list, cut on the host: the segments one wave serves, then those that take a workgroup (each in map order) ----
    int32_t* items = nullptr;
    HIPCHK(c, c->segStage.stage((size_t)N, &items));
    int32_t nShort = 0;
    for (int32_t i = 0; i < N; ++i) if (seg_off_host[i + 1] - seg_off_host[i] < (int64_t)c->seg_block_min) items[nShort++] = i;
    int32_t nLong = 0;
    for (int32_t i = 0; i < N; ++i) if (seg_off_host[i + 1] - seg_off_host[i] >= (int64_t)c->seg_block_min) items[nShort + nLong++] = i;
    HIPCHK(c, c->segStage.upload(c->segItems, (size_t)N, c->stream));
    const SegShapeArgs A{points, seg_off_dev, c->segItems.as<int32_t>(), out, status, (int)params->center_ref, (int)params->out_stride,
                         (int)params->col_center, (int)params->col_pca, (int)params->col_volume, (int)params->col_extent};
    if (nShort) hipLaunchKernelGGL(k_seg_shapes_wave, dim3((unsigned)((nShort + 3) / 4)), dim3(256), 0, c->stream, A, (int)nShort);
    if (nLong) hipLaunchKernelGGL(k_seg_shapes_block, dim3((unsigned)nLong), dim3(256), 0, c->stream, A, (int)nShort);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_segment_shapes(roman_ctx_t* c, const double* points, const int64_t* seg_off, int32_t N, const roman_segment_shape_params_t* params,
                         double* out, int32_t* status)
{
    int64_t P = 0;
    int rc = segment_shapes_check(c, points, seg_off, N, params, out, status, &P);
    if (rc || N == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HostMirror m(c);
    const auto dPts = m.in(points, sizeof(double) * 3 * (size_t)P);
    const auto dOff = m.in(seg_off, sizeof(int64_t) * ((size_t)N + 1));
    const auto dOut = m.inout(out, sizeof(double) * (size_t)N * (size_t)params->out_stride);
    const auto dSt = m.out(status, sizeof(int32_t) * (size_t)N);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_segment_shapes_dev(c, P ? dPts.dev() : reinterpret_cast<const double*>(dOff.dev()) /* never read: every segment is empty */, dOff.dev(),
                                  seg_off, N, params, dOut.dev(), dSt.dev());
    if (rc) return rc;
    return m.download();
}

int roman_ctx_set_segment_block_min(roman_ctx_t* c, int32_t n)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (n < 0) return fail(c, ROMAN_E_INVALID, "n must be >= 0 (0: the default)");
    c->seg_block_min = n ? n : SEG_BLOCK_MIN;
    return ROMAN_OK;
}

// --- frame data association: voxel IoU / IoM, cosine and score of every cloud pair ---------------------------------
static_assert(ASSOC_ST_OK == ROMAN_ASSOC_OK && ASSOC_ST_EMPTY == ROMAN_ASSOC_EMPTY && ASSOC_ST_RANGE == ROMAN_ASSOC_RANGE &&
              ASSOC_WAVE_MAX == ROMAN_ASSOC_WAVE_MAX && ASSOC_LDS_MAX == ROMAN_ASSOC_LDS_MAX, "kernels.hip.h and roman_hip.h name the same numbers");
static_assert(sizeof(roman_assoc_params_t) == 48, "roman_assoc_params_t: a double, two int32 words, four doubles");
static_assert(ASSOC_WAVE_MAX <= ASSOC_WAVE_CAP && ASSOC_LDS_MAX <= ASSOC_LDS_CAP, "a cut cannot exceed the LDS its kernel sorts in");

struct AssocSizes { int64_t P; int32_t clouds, cols, col0; };

// Everything roman_assoc_scores* judge on host memory.  The argument checks come first and the context last, so that each of them
// answers without a device (a NULL context then leaves the text with roman_last_error(NULL)).
static int assoc_check(roman_ctx* c, const roman_assoc_params_t* P, const void* points, const int64_t* cloud_off, int32_t N1, int32_t N2,
                       const void* desc, int32_t d, const void* geo, const void* score, const void* status, AssocSizes* Z)
{
    if (!P) return fail(c, ROMAN_E_INVALID, "params is NULL");
    if (!(P->voxel_size > 0.0) || !std::isfinite(P->voxel_size)) return fail(c, ROMAN_E_INVALID, "voxel_size must be finite and > 0 (got %g)", P->voxel_size);
    if (P->geometric != ROMAN_ASSOC_IOU && P->geometric != ROMAN_ASSOC_IOM) return fail(c, ROMAN_E_INVALID, "unknown geometric method %d", P->geometric);
    if (P->semantic != 0 && P->semantic != 1) return fail(c, ROMAN_E_INVALID, "semantic must be 0 or 1 (got %d)", P->semantic);
    if (!(P->geo_range[1] != P->geo_range[0]) || P->geo_range[0] != P->geo_range[0])
        return fail(c, ROMAN_E_INVALID, "geo_range = (%g, %g): threshold and maximum must differ", P->geo_range[0], P->geo_range[1]);
    if (P->semantic && (!(P->sem_range[1] != P->sem_range[0]) || P->sem_range[0] != P->sem_range[0]))
        return fail(c, ROMAN_E_INVALID, "sem_range = (%g, %g): threshold and maximum must differ", P->sem_range[0], P->sem_range[1]);
    if (N1 < 0 || N2 < -1) return fail(c, ROMAN_E_INVALID, "N1 = %d, N2 = %d: N1 >= 0 and N2 >= 0, or N2 == -1 for self mode", N1, N2);
    if (N1 > (1 << 30) || N2 > (1 << 30) - N1) return fail(c, ROMAN_E_TOO_LARGE, "more than 2^30 clouds");
    Z->clouds = N2 < 0 ? N1 : N1 + N2; Z->cols = N2 < 0 ? N1 : N2; Z->col0 = N2 < 0 ? 0 : N1;
    if ((int64_t)N1 * Z->cols > (int64_t)(1 << 30)) return fail(c, ROMAN_E_TOO_LARGE, "%d x %d: more than 2^30 pairs", N1, Z->cols);
    if (!cloud_off) return fail(c, ROMAN_E_INVALID, "cloud_off is NULL");
    { const int rc = cloud_offsets_check(c, cloud_off, Z->clouds, "cloud_off", "cloud"); if (rc) return rc; }
    Z->P = cloud_off[Z->clouds];
    if (d < 0) return fail(c, ROMAN_E_INVALID, "d < 0");
    if (P->semantic && d > 0 && !desc && Z->clouds > 0) return fail(c, ROMAN_E_INVALID, "desc is NULL with d = %d", d);
    if (P->semantic && d == 0 && desc) return fail(c, ROMAN_E_INVALID, "desc is given with d = 0");
    if (Z->P > 0 && !points) return fail(c, ROMAN_E_INVALID, "points is NULL");
    if (N1 > 0 && Z->cols > 0 && (!geo || !score || !status)) return fail(c, ROMAN_E_INVALID, "geo / score / status is NULL");
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    return ROMAN_OK;
}

int roman_assoc_scores_dev(roman_ctx_t* c, const roman_assoc_params_t* params, const double* points, const int64_t* cloud_off_dev,
                           const int64_t* cloud_off_host, int32_t N1, int32_t N2, const double* desc, int32_t d,
                           int32_t* n_vox, int32_t* inter, double* geo, double* sem, double* score, int32_t* status)
{
    AssocSizes Z{};
    int rc = assoc_check(c, params, points, cloud_off_host, N1, N2, desc, d, geo, score, status, &Z);
    if (rc) return rc;
    if (N1 == 0 || Z.cols == 0) return ROMAN_OK;
    if (!cloud_off_dev) return fail(c, ROMAN_E_INVALID, "cloud_off is NULL on the device");
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t NC = Z.clouds;
    const bool cosine = params->semantic && d > 0;
    // ---- the workspace, from the host offsets alone ----
    HIPCHK(c, c->asKeys.ensure(sizeof(unsigned long long) * (size_t)std::max<int64_t>(Z.P, 1)));
    HIPCHK(c, c->asRec.ensure(sizeof(AssocCloud) * (size_t)NC));
    if (cosine) HIPCHK(c, c->asNorm.ensure(sizeof(double) * (size_t)NC));
    // ---- the list, cut on the host: the clouds of one wave, of a workgroup sorting in LDS, of a workgroup that merges ----
    const int64_t cutW = c->assoc_wave_max, cutL = c->assoc_lds_max;
    int32_t* items = nullptr;
    HIPCHK(c, c->asStage.stage((size_t)NC, &items));
    int32_t nW = 0, nL = 0, nM = 0;
    int64_t longest = 0;
    for (int32_t i = 0; i < NC; ++i) if (cloud_off_host[i + 1] - cloud_off_host[i] <= cutW) items[nW++] = i;
    for (int32_t i = 0; i < NC; ++i) { const int64_t n = cloud_off_host[i + 1] - cloud_off_host[i]; if (n > cutW && n <= cutL) items[nW + nL++] = i; }
    for (int32_t i = 0; i < NC; ++i) { const int64_t n = cloud_off_host[i + 1] - cloud_off_host[i]; if (n > cutL) { items[nW + nL + nM++] = i; longest = std::max(longest, n); } }
    if (nM) HIPCHK(c, c->asScratch.ensure(sizeof(unsigned long long) * (size_t)Z.P));
    HIPCHK(c, c->asStage.upload(c->asItems, (size_t)NC, c->stream));
    const AssocKeyArgs K{points, cloud_off_dev, c->asItems.as<int32_t>(), c->asKeys.as<unsigned long long>(), c->asScratch.as<unsigned long long>(),
                         c->asRec.as<AssocCloud>(), n_vox, status, params->voxel_size, (int)cutL};
    if (nW) hipLaunchKernelGGL(k_assoc_keys_wave, dim3((unsigned)((nW + 3) / 4)), dim3(256), 0, c->stream, K, (int)nW);
    if (nL) hipLaunchKernelGGL(k_assoc_keys_block<false>, dim3((unsigned)nL), dim3(256), 0, c->stream, K, (int)nW);
    if (nM) hipLaunchKernelGGL(k_assoc_keys_block<true>, dim3((unsigned)nM), dim3(256), 0, c->stream, K, (int)(nW + nL));
    if (cosine) hipLaunchKernelGGL(k_assoc_norms, dim3((unsigned)((NC + 3) / 4)), dim3(256), 0, c->stream, desc, (int)d, (int)NC, c->asNorm.as<double>());
    const AssocPairArgs A{c->asRec.as<AssocCloud>(), c->asKeys.as<unsigned long long>(), cloud_off_dev, cosine ? desc : nullptr, c->asNorm.as<double>(),
                          cosine ? (int)d : 0, (int)N1, (int)Z.cols, (int)Z.col0, params->geometric == ROMAN_ASSOC_IOM ? 1 : 0, (int)params->semantic,
                          std::pow(params->voxel_size, 3.0) /* voxel_size**3 as Python's float power gives it */,
                          params->geo_range[0], params->geo_range[1], params->sem_range[0], params->sem_range[1], inter, geo, sem, score};
    const int64_t pairs = (int64_t)N1 * Z.cols;
    hipLaunchKernelGGL(k_assoc_pairs, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, c->stream, A);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_assoc_scores(roman_ctx_t* c, const roman_assoc_params_t* params, const double* points, const int64_t* cloud_off,
                       int32_t N1, int32_t N2, const double* desc, int32_t d,
                       int32_t* n_vox, int32_t* inter, double* geo, double* sem, double* score, int32_t* status)
{
    AssocSizes Z{};
    int rc = assoc_check(c, params, points, cloud_off, N1, N2, desc, d, geo, score, status, &Z);
    if (rc || N1 == 0 || Z.cols == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const size_t NC = (size_t)Z.clouds, pairs = (size_t)N1 * (size_t)Z.cols;
    const bool cosine = params->semantic && d > 0;
    HostMirror m(c);
    const auto dPts = m.in(points, sizeof(double) * 3 * (size_t)Z.P);
    const auto dOff = m.in(cloud_off, sizeof(int64_t) * (NC + 1));
    const auto dDesc = m.in(desc, cosine ? sizeof(double) * NC * (size_t)d : 0);
    const auto dNv = m.out(n_vox, n_vox ? sizeof(int32_t) * NC : 0);
    const auto dSt = m.out(status, sizeof(int32_t) * NC);
    const auto dIn = m.out(inter, inter ? sizeof(int32_t) * pairs : 0);
    const auto dGeo = m.out(geo, sizeof(double) * pairs);
    const auto dSem = m.out(sem, (sem && params->semantic) ? sizeof(double) * pairs : 0);
    const auto dSc = m.out(score, sizeof(double) * pairs);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_assoc_scores_dev(c, params, Z.P ? dPts.dev() : reinterpret_cast<const double*>(dOff.dev()) /* never read: every cloud is empty */, dOff.dev(),
                                cloud_off, N1, N2, dDesc.dev(), cosine ? d : 0, dNv.dev(), dIn.dev(), dGeo.dev(), dSem.dev(), dSc.dev(), dSt.dev());
    if (rc) return rc;
    return m.download();
}

int roman_ctx_set_assoc_cuts(roman_ctx_t* c, int32_t wave_max, int32_t lds_max)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const int w = wave_max ? wave_max : ASSOC_WAVE_MAX, l = lds_max ? lds_max : ASSOC_LDS_MAX;
    if (wave_max < 0 || lds_max < 0 || w > ASSOC_WAVE_CAP || l > ASSOC_LDS_CAP || l < 2 || w > l)
        return fail(c, ROMAN_E_INVALID, "wave_max = %d, lds_max = %d: 0 <= wave_max <= %d, wave_max <= lds_max, 2 <= lds_max <= %d (0: the default)",
                    wave_max, lds_max, ASSOC_WAVE_CAP, ASSOC_LDS_CAP);
    c->assoc_wave_max = w; c->assoc_lds_max = l;
    return ROMAN_OK;
}

// --- segment update: integrate, down-sample, prune outliers for a list of jobs -------------------------------------
static_assert(INTEG_WAVE_MAX == ROMAN_INTEGRATE_WAVE_MAX && INTEG_LDS_MAX == ROMAN_INTEGRATE_LDS_MAX && INTEG_NEIGHBORS == ROMAN_INTEGRATE_NEIGHBORS,
              "kernels.hip.h and roman_hip.h name the same numbers");
static_assert(sizeof(roman_integrate_params_t) == 24 && sizeof(roman_integrate_job_t) == 12 && sizeof(IntegJob) == sizeof(roman_integrate_job_t),
              "roman_integrate_params_t: two doubles and an int32 word; roman_integrate_job_t: three int32 words");
constexpr int64_t INTEG_JOB_MAX = 1ll << 28;    // points of one job: the kernels index 3 * point in 32 bits

// Everything roman_segment_integrate* judge on host memory -> *total: the points of all slots.  The argument checks come first and
// the context last, so that each of them answers without a device.
static int integrate_check(roman_ctx* c, const roman_integrate_params_t* P, const void* points, const int64_t* cloud_off, int32_t n_clouds,
                           const void* poses, int32_t n_poses, const roman_integrate_job_t* jobs, int32_t n_jobs,
                           const void* out_points, const void* out_count, const void* out_status, int64_t* total)
{
    if (!P) return fail(c, ROMAN_E_INVALID, "params is NULL");
    if (!(P->voxel_size > 0.0) || !std::isfinite(P->voxel_size)) return fail(c, ROMAN_E_INVALID, "voxel_size must be finite and > 0 (got %g)", P->voxel_size);
    if (P->outlier_std != P->outlier_std) return fail(c, ROMAN_E_INVALID, "outlier_std is NaN (not finite or <= 0: no outlier removal)");
    if (P->nb_neighbors != ROMAN_INTEGRATE_NEIGHBORS) return fail(c, ROMAN_E_INVALID, "nb_neighbors must be %d (got %d)", ROMAN_INTEGRATE_NEIGHBORS, P->nb_neighbors);
    if (n_clouds < 0 || n_poses < 0 || n_jobs < 0) return fail(c, ROMAN_E_INVALID, "n_clouds = %d, n_poses = %d, n_jobs = %d: none may be negative", n_clouds, n_poses, n_jobs);
    if (!cloud_off) return fail(c, ROMAN_E_INVALID, "cloud_off is NULL");
    { const int rc = cloud_offsets_check(c, cloud_off, n_clouds, "cloud_off", "cloud"); if (rc) return rc; }
    if (n_jobs > 0 && !jobs) return fail(c, ROMAN_E_INVALID, "jobs is NULL");
    std::vector<char> named((size_t)n_clouds, 0);
    bool posed = false;
    *total = 0;
    for (int32_t j = 0; j < n_jobs; ++j) {
        const roman_integrate_job_t& J = jobs[j];
        if (J.add < 0 || J.add >= n_clouds) return fail(c, ROMAN_E_INVALID, "job %d: add = %d is not one of the %d clouds", j, J.add, n_clouds);
        if (J.base < -1 || J.base >= n_clouds) return fail(c, ROMAN_E_INVALID, "job %d: base = %d is neither -1 nor one of the %d clouds", j, J.base, n_clouds);
        if (J.pose < -1 || J.pose >= n_poses) return fail(c, ROMAN_E_INVALID, "job %d: pose = %d is neither -1 nor one of the %d poses", j, J.pose, n_poses);
        if (J.base >= 0) {
            if (named[(size_t)J.base]) return fail(c, ROMAN_E_INVALID, "job %d: base cloud %d is the base of an earlier job", j, J.base);
            named[(size_t)J.base] = 1;
        }
        posed = posed || J.pose >= 0;
        const int64_t n = (J.base >= 0 ? cloud_off[J.base + 1] - cloud_off[J.base] : 0) + (cloud_off[J.add + 1] - cloud_off[J.add]);
        if (n > INTEG_JOB_MAX) return fail(c, ROMAN_E_TOO_LARGE, "job %d holds more than 2^28 points", j);
        *total += n;
    }
    if (posed && !poses) return fail(c, ROMAN_E_INVALID, "poses is NULL and a job names one");
    if (cloud_off[n_clouds] > 0 && !points) return fail(c, ROMAN_E_INVALID, "points is NULL");
    if (n_jobs > 0 && (!out_count || !out_status || (*total > 0 && !out_points))) return fail(c, ROMAN_E_INVALID, "out_points / out_count / out_status is NULL");
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    return ROMAN_OK;
}

static inline bool integrate_outlier(const roman_integrate_params_t* P) { return P->outlier_std > 0.0 && std::isfinite(P->outlier_std); }

int roman_segment_integrate_dev(roman_ctx_t* c, const roman_integrate_params_t* params, const double* points, const int64_t* cloud_off_dev,
                                const int64_t* cloud_off_host, int32_t n_clouds, const double* poses, int32_t n_poses,
                                const roman_integrate_job_t* jobs_dev, const roman_integrate_job_t* jobs_host, int32_t n_jobs,
                                double* out_points, int32_t* out_count, int32_t* out_status, double* out_avg, double* out_thr)
{
    int64_t total = 0;
    int rc = integrate_check(c, params, points, cloud_off_host, n_clouds, poses, n_poses, jobs_host, n_jobs, out_points, out_count, out_status, &total);
    if (rc || n_jobs == 0) return rc;
    if (!cloud_off_dev) return fail(c, ROMAN_E_INVALID, "cloud_off is NULL on the device");
    if (!jobs_dev) return fail(c, ROMAN_E_INVALID, "jobs is NULL on the device");
    HIPCHK(c, hipSetDevice(c->device));
    const bool outlier = integrate_outlier(params);
    const int64_t cutW = c->integ_wave_max, cutL = c->integ_lds_max;
    auto size_of = [&](int32_t j) {
        const roman_integrate_job_t& J = jobs_host[j];
        return (J.base >= 0 ? cloud_off_host[J.base + 1] - cloud_off_host[J.base] : 0) + (cloud_off_host[J.add + 1] - cloud_off_host[J.add]);
    };
    auto cleaned = [&](int32_t j) { return outlier && cloud_off_host[jobs_host[j].add + 1] > cloud_off_host[jobs_host[j].add]; };
    // ---- the tables, cut on the host: slot offsets | the jobs of one wave, of a workgroup in LDS, of a workgroup that merges | the
    // query tiles of the two workgroup classes (none for a job whose added cloud is empty: it has no clean-up) ----
    size_t n_tiles = 0;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) > cutW && cleaned(j)) n_tiles += (size_t)((size_of(j) + INTEG_TILE - 1) / INTEG_TILE);
    const size_t oItems = (size_t)n_jobs + 1, oTiles = oItems + (size_t)n_jobs, n_tab = oTiles + n_tiles;
    int64_t* tab = nullptr;
    HIPCHK(c, c->sgStage.stage(n_tab, &tab));
    tab[0] = 0;
    for (int32_t j = 0; j < n_jobs; ++j) tab[j + 1] = tab[j] + size_of(j);
    int32_t nW = 0, nL = 0, nM = 0;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) <= cutW) tab[oItems + nW++] = j;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) > cutW && size_of(j) <= cutL) tab[oItems + nW + nL++] = j;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) > cutL) tab[oItems + nW + nL + nM++] = j;
    size_t t = oTiles;
    for (int32_t k = nW; k < n_jobs; ++k) {
        const int32_t j = (int32_t)tab[oItems + k];
        if (!cleaned(j)) continue;
        for (int64_t q = 0; q * INTEG_TILE < size_of(j); ++q) tab[t++] = ((int64_t)j << 32) | q;
    }
    // ---- the workspace, from the host offsets alone ----
    const size_t room = (size_t)std::max<int64_t>(total, 1);
    HIPCHK(c, c->sgPts.ensure(sizeof(double) * 3 * room));
    if (nM) {
        HIPCHK(c, c->sgKeys.ensure(sizeof(unsigned long long) * room)); HIPCHK(c, c->sgKeys2.ensure(sizeof(unsigned long long) * room));
        HIPCHK(c, c->sgIdx.ensure(sizeof(int32_t) * room)); HIPCHK(c, c->sgIdx2.ensure(sizeof(int32_t) * room));
    }
    if (outlier) HIPCHK(c, c->sgDs.ensure(sizeof(double) * 3 * room));
    if (outlier && !out_avg) HIPCHK(c, c->sgAvg.ensure(sizeof(double) * room));
    HIPCHK(c, c->sgM.ensure(sizeof(int32_t) * (size_t)n_jobs));
    HIPCHK(c, c->sgStage.upload(c->sgItems, n_tab, c->stream));
    const int64_t* dTab = c->sgItems.as<int64_t>();
    IntegArgs A{points, cloud_off_dev, poses, reinterpret_cast<const IntegJob*>(jobs_dev), dTab, dTab + oItems,
                c->sgPts.as<double>(), c->sgDs.as<double>(), c->sgKeys.as<unsigned long long>(), c->sgKeys2.as<unsigned long long>(),
                c->sgIdx.as<int32_t>(), c->sgIdx2.as<int32_t>(), c->sgM.as<int32_t>(), out_avg ? out_avg : c->sgAvg.as<double>(),
                out_points, out_count, out_status, out_thr, params->voxel_size, params->outlier_std, outlier ? 1 : 0, (int)cutL};
    if (nW) hipLaunchKernelGGL(k_integ_front_wave, dim3((unsigned)nW), dim3(64), 0, c->stream, A);
    if (nL) hipLaunchKernelGGL(k_integ_front_block<false>, dim3((unsigned)nL), dim3(256), 0, c->stream, A, (int)nW);
    if (nM) hipLaunchKernelGGL(k_integ_front_block<true>, dim3((unsigned)nM), dim3(256), 0, c->stream, A, (int)(nW + nL));
    if (outlier) {
        if (nW) hipLaunchKernelGGL(k_integ_knn_wave, dim3((unsigned)((nW + 3) / 4)), dim3(256), 0, c->stream, A, (int)nW);
        if (n_tiles) hipLaunchKernelGGL(k_integ_knn_tile, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, A, (int)n_jobs);
        if (nW) hipLaunchKernelGGL(k_integ_finish_wave, dim3((unsigned)((nW + 3) / 4)), dim3(256), 0, c->stream, A, (int)nW);
        if (nL + nM) hipLaunchKernelGGL(k_integ_finish_block, dim3((unsigned)(nL + nM)), dim3(256), 0, c->stream, A, (int)nW);
    }
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_segment_integrate(roman_ctx_t* c, const roman_integrate_params_t* params, const double* points, const int64_t* cloud_off, int32_t n_clouds,
                            const double* poses, int32_t n_poses, const roman_integrate_job_t* jobs, int32_t n_jobs,
                            double* out_points, int32_t* out_count, int32_t* out_status, double* out_avg, double* out_thr)
{
    int64_t total = 0;
    int rc = integrate_check(c, params, points, cloud_off, n_clouds, poses, n_poses, jobs, n_jobs, out_points, out_count, out_status, &total);
    if (rc || n_jobs == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const bool outlier = integrate_outlier(params);
    HostMirror m(c);
    const auto dPts = m.in(points, sizeof(double) * 3 * (size_t)cloud_off[n_clouds]);
    const auto dOff = m.in(cloud_off, sizeof(int64_t) * ((size_t)n_clouds + 1));
    const auto dPose = m.in(poses, poses ? sizeof(double) * 16 * (size_t)n_poses : 0);
    const auto dJobs = m.in(jobs, sizeof(roman_integrate_job_t) * (size_t)n_jobs);
    // what a job leaves untouched — its slot past out_count, a threshold it does not form — comes back as the caller had it
    const auto dOut = m.inout(out_points, sizeof(double) * 3 * (size_t)total);
    const auto dCnt = m.out(out_count, sizeof(int32_t) * (size_t)n_jobs);
    const auto dSt = m.out(out_status, sizeof(int32_t) * (size_t)n_jobs);
    const auto dAvg = m.inout(out_avg, (out_avg && outlier) ? sizeof(double) * (size_t)total : 0);
    const auto dThr = m.inout(out_thr, (out_thr && outlier) ? sizeof(double) * (size_t)n_jobs : 0);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_segment_integrate_dev(c, params, dPts.dev(), dOff.dev(), cloud_off, n_clouds, dPose.dev(), n_poses, dJobs.dev(), jobs, n_jobs,
                                     dOut.dev() /* NULL when every slot is empty */, dCnt.dev(), dSt.dev(), dAvg.dev(), dThr.dev());
    if (rc) return rc;
    return m.download();
}

int roman_ctx_set_integrate_cuts(roman_ctx_t* c, int32_t wave_max, int32_t lds_max)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const int w = wave_max ? wave_max : INTEG_WAVE_MAX, l = lds_max ? lds_max : INTEG_LDS_MAX;
    if (wave_max < 0 || lds_max < 0 || l > INTEG_LDS_CAP || l < 2 || w > l)
        return fail(c, ROMAN_E_INVALID, "wave_max = %d, lds_max = %d: 0 <= wave_max <= lds_max, 2 <= lds_max <= %d (0: the default)", wave_max, lds_max, INTEG_LDS_CAP);
    c->integ_wave_max = w; c->integ_lds_max = l;
    return ROMAN_OK;
}

// --- segment clustering: final_cleanup's DBSCAN and "keep the largest cluster" for a list of jobs ---------------
static_assert(CLUS_WAVE_MAX == ROMAN_CLUSTER_WAVE_MAX && CLUS_LDS_MAX == ROMAN_CLUSTER_LDS_MAX && CLUS_TILE == ROMAN_CLUSTER_TILE && CLUS_COLS == ROMAN_CLUSTER_COLS,
              "kernels.hip.h and roman_hip.h name the same numbers");
static_assert(sizeof(roman_cluster_params_t) == 16, "roman_cluster_params_t: a double and an int32 word");
constexpr int64_t CLUS_CALL_MAX = 1ll << 28;    // points of one call: the kernels index 3 * point in 32 bits inside a job, the slots in 64

// Everything roman_segment_cluster* judge on host memory -> *total: the points of all slots.  The argument checks come first and
// the context last, so that each of them answers without a device.
static int cluster_check(roman_ctx* c, const roman_cluster_params_t* P, const void* points, const int64_t* cloud_off, int32_t n_clouds,
                         const int32_t* jobs, int32_t n_jobs, const void* out_points, const void* out_count, const void* out_status,
                         const void* out_n_clusters, int64_t* total)
{
    if (!P) return fail(c, ROMAN_E_INVALID, "params is NULL");
    if (!(P->eps > 0.0) || !std::isfinite(P->eps)) return fail(c, ROMAN_E_INVALID, "eps must be finite and > 0 (got %g)", P->eps);
    if (P->min_points < 1) return fail(c, ROMAN_E_INVALID, "min_points must be >= 1 (got %d)", P->min_points);
    if (n_clouds < 0 || n_jobs < 0) return fail(c, ROMAN_E_INVALID, "n_clouds = %d, n_jobs = %d: none may be negative", n_clouds, n_jobs);
    if (!cloud_off) return fail(c, ROMAN_E_INVALID, "cloud_off is NULL");
    { const int rc = cloud_offsets_check(c, cloud_off, n_clouds, "cloud_off", "cloud"); if (rc) return rc; }
    if (n_jobs > 0 && !jobs) return fail(c, ROMAN_E_INVALID, "jobs is NULL");
    std::vector<char> named((size_t)n_clouds, 0);
    *total = 0;
    for (int32_t j = 0; j < n_jobs; ++j) {
        if (jobs[j] < 0 || jobs[j] >= n_clouds) return fail(c, ROMAN_E_INVALID, "job %d: %d is not one of the %d clouds", j, jobs[j], n_clouds);
        if (named[(size_t)jobs[j]]) return fail(c, ROMAN_E_INVALID, "job %d: cloud %d is named by an earlier job", j, jobs[j]);
        named[(size_t)jobs[j]] = 1;
        *total += cloud_off[jobs[j] + 1] - cloud_off[jobs[j]];
    }
    if (*total > CLUS_CALL_MAX) return fail(c, ROMAN_E_TOO_LARGE, "the jobs hold more than 2^28 points");
    if (cloud_off[n_clouds] > 0 && !points) return fail(c, ROMAN_E_INVALID, "points is NULL");
    if (n_jobs > 0 && (!out_count || !out_status || !out_n_clusters || (*total > 0 && !out_points)))
        return fail(c, ROMAN_E_INVALID, "out_points / out_count / out_status / out_n_clusters is NULL");
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    return ROMAN_OK;
}

int roman_segment_cluster_dev(roman_ctx_t* c, const roman_cluster_params_t* params, const double* points, const int64_t* cloud_off_dev,
                              const int64_t* cloud_off_host, int32_t n_clouds, const int32_t* jobs_dev, const int32_t* jobs_host, int32_t n_jobs,
                              double* out_points, int32_t* out_count, int32_t* out_status, int32_t* out_labels, int32_t* out_n_clusters, int32_t* out_kept)
{
    int64_t total = 0;
    int rc = cluster_check(c, params, points, cloud_off_host, n_clouds, jobs_host, n_jobs, out_points, out_count, out_status, out_n_clusters, &total);
    if (rc || n_jobs == 0) return rc;
    if (!cloud_off_dev) return fail(c, ROMAN_E_INVALID, "cloud_off is NULL on the device");
    if (!jobs_dev) return fail(c, ROMAN_E_INVALID, "jobs is NULL on the device");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t cutW = c->clus_wave_max, cutL = c->clus_lds_max;
    auto size_of = [&](int32_t j) { return cloud_off_host[jobs_host[j] + 1] - cloud_off_host[jobs_host[j]]; };
    // ---- the tables, cut on the host: slot offsets | the jobs of one wave, of a workgroup in LDS, of the tiled class | its query tiles ----
    size_t n_tiles = 0;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) > cutL) n_tiles += (size_t)((size_of(j) + CLUS_TILE - 1) / CLUS_TILE);
    const size_t oItems = (size_t)n_jobs + 1, oTiles = oItems + (size_t)n_jobs, n_tab = oTiles + n_tiles;
    int64_t* tab = nullptr;
    HIPCHK(c, c->clStage.stage(n_tab, &tab));
    tab[0] = 0;
    for (int32_t j = 0; j < n_jobs; ++j) tab[j + 1] = tab[j] + size_of(j);
    int32_t nW = 0, nL = 0, nT = 0;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) <= cutW) tab[oItems + nW++] = j;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) > cutW && size_of(j) <= cutL) tab[oItems + nW + nL++] = j;
    for (int32_t j = 0; j < n_jobs; ++j) if (size_of(j) > cutL) tab[oItems + nW + nL + nT++] = j;
    size_t t = oTiles;
    for (int32_t k = nW + nL; k < n_jobs; ++k) {
        const int32_t j = (int32_t)tab[oItems + k];
        for (int64_t q = 0; q * CLUS_TILE < size_of(j); ++q) tab[t++] = ((int64_t)j << 32) | q;
    }
    // ---- the workspace, from the host offsets alone ----
    const size_t room = sizeof(int32_t) * (size_t)std::max<int64_t>(total, 1);
    if (nT) { HIPCHK(c, c->clPar.ensure(room)); HIPCHK(c, c->clAux.ensure(room)); HIPCHK(c, c->clHist.ensure(room)); }
    if (!out_labels) HIPCHK(c, c->clLab.ensure(room));
    HIPCHK(c, c->clStage.upload(c->clItems, n_tab, c->stream));
    const int64_t* dTab = c->clItems.as<int64_t>();
    const ClusArgs A{points, cloud_off_dev, jobs_dev, dTab, dTab + oItems, c->clPar.as<int32_t>(), c->clAux.as<int32_t>(), c->clHist.as<int32_t>(),
                     out_labels ? out_labels : c->clLab.as<int32_t>(), out_points, out_count, out_status, out_n_clusters, out_kept,
                     params->eps * params->eps, (int)params->min_points};
    if (nW) hipLaunchKernelGGL(k_clus_wave, dim3((unsigned)((nW + 3) / 4)), dim3(256), 0, c->stream, A, (int)nW);
    if (nL) hipLaunchKernelGGL(k_clus_block, dim3((unsigned)nL), dim3(256), 0, c->stream, A, (int)nW);
    if (nT) {
        hipLaunchKernelGGL(k_clus_tile<0>, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, A, (int)n_jobs);
        hipLaunchKernelGGL(k_clus_tile<1>, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, A, (int)n_jobs);
        hipLaunchKernelGGL(k_clus_tile<2>, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, A, (int)n_jobs);
        hipLaunchKernelGGL(k_clus_finish_block, dim3((unsigned)nT), dim3(256), 0, c->stream, A, (int)(nW + nL));
    }
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_segment_cluster(roman_ctx_t* c, const roman_cluster_params_t* params, const double* points, const int64_t* cloud_off, int32_t n_clouds,
                          const int32_t* jobs, int32_t n_jobs, double* out_points, int32_t* out_count, int32_t* out_status,
                          int32_t* out_labels, int32_t* out_n_clusters, int32_t* out_kept)
{
    int64_t total = 0;
    int rc = cluster_check(c, params, points, cloud_off, n_clouds, jobs, n_jobs, out_points, out_count, out_status, out_n_clusters, &total);
    if (rc || n_jobs == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HostMirror m(c);
    const auto dPts = m.in(points, sizeof(double) * 3 * (size_t)cloud_off[n_clouds]);
    const auto dOff = m.in(cloud_off, sizeof(int64_t) * ((size_t)n_clouds + 1));
    const auto dJobs = m.in(jobs, sizeof(int32_t) * (size_t)n_jobs);
    // what a job leaves untouched — its slot past out_count, the labels of a RANGE job — comes back as the caller had it
    const auto dOut = m.inout(out_points, sizeof(double) * 3 * (size_t)total);
    const auto dCnt = m.out(out_count, sizeof(int32_t) * (size_t)n_jobs);
    const auto dSt = m.out(out_status, sizeof(int32_t) * (size_t)n_jobs);
    const auto dLab = m.inout(out_labels, out_labels ? sizeof(int32_t) * (size_t)total : 0);
    const auto dNc = m.out(out_n_clusters, sizeof(int32_t) * (size_t)n_jobs);
    const auto dKept = m.out(out_kept, out_kept ? sizeof(int32_t) * (size_t)n_jobs : 0);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_segment_cluster_dev(c, params, dPts.dev(), dOff.dev(), cloud_off, n_clouds, dJobs.dev(), jobs, n_jobs,
                                   dOut.dev() /* NULL when every slot is empty */, dCnt.dev(), dSt.dev(), dLab.dev(), dNc.dev(), dKept.dev());
    if (rc) return rc;
    return m.download();
}

int roman_ctx_set_cluster_cuts(roman_ctx_t* c, int32_t wave_max, int32_t lds_max)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const int w = wave_max ? wave_max : CLUS_WAVE_MAX, l = lds_max ? lds_max : CLUS_LDS_MAX;
    if (wave_max < 0 || lds_max < 0 || w > CLUS_WAVE_MAX || l > CLUS_LDS_CAP || w > l)
        return fail(c, ROMAN_E_INVALID, "wave_max = %d, lds_max = %d: 0 <= wave_max <= %d, wave_max <= lds_max <= %d (0: the default)",
                    wave_max, lds_max, CLUS_WAVE_MAX, CLUS_LDS_CAP);
    c->clus_wave_max = w; c->clus_lds_max = l;
    return ROMAN_OK;
}

// What the grid gate and the session gate ask of roman_grid_gate_params_t, in front of their own checks.  The caller's check of its
// counts (`bad_sizes`, with the text `sizes`) is handed in because it has always been the THIRD check, between the given similarity
// and the reserved words, and a call wrong in two ways keeps its answer.  `aabb_entry`: the entry points that serve a missing radius
static int gate_params_check(roman_ctx* c, const roman_grid_gate_params_t* P, bool sim_in, bool aabb, const char* aabb_entry, bool bad_sizes, const char* sizes)
{
    if (!P) return fail(c, ROMAN_E_INVALID, "gparams is NULL");
    if (sim_in && P->desc_dim != 0) return fail(c, ROMAN_E_INVALID, "desc_dim=%d: the similarity is given, desc_dim must be 0", P->desc_dim);
    if (bad_sizes) return fail(c, ROMAN_E_INVALID, "%s", sizes);
    if (P->reserved0 != 0 || P->reserved1 != 0 || P->reserved[0] != 0 || P->reserved[1] != 0)
        return fail(c, ROMAN_E_INVALID, "roman_grid_gate_params_t reserved words must be 0");
    if (!aabb && P->radius != P->radius) return fail(c, ROMAN_E_INVALID, "radius is NaN");
    if (P->desc_dim < 0) return fail(c, ROMAN_E_INVALID, "desc_dim=%d is negative", P->desc_dim);
    if (!aabb && P->radius < 0.0) return fail(c, ROMAN_E_UNSUPPORTED, "radius=%g: without a radius the gate is the AABB test (%s)", P->radius, aabb_entry);
    return ROMAN_OK;
}

// the instantiation of a gate kernel for (sim_in, aabb)
static auto grid_gate_kernel(bool sim_in, bool aabb)
{
    return sim_in ? (aabb ? k_grid_gate<true, true> : k_grid_gate<true, false>) : (aabb ? k_grid_gate<false, true> : k_grid_gate<false, false>);
}

static auto session_gate_kernel(bool sim_in, bool aabb)
{
    using Kernel = void (*)(roman_grid_gate_params_t, SessionTab, int64_t, GridSide, const double*, GridOut);
    const Kernel radius = sim_in ? k_session_gate<true> : k_session_gate<false>, boxes = sim_in ? k_session_gate<true, true> : k_session_gate<false, true>;
    return aabb ? boxes : radius;
}

// --- the gates' argument blocks: what one gate call works on, under names, from the C entry point to the launch ---------------------
// An entry point fills one from its own parameters; a host form hands the device form a copy whose arrays are the mirror's.
// sim_in: out.sim holds every pair's similarity already and is only read, desc is not; aabb: NEARBY from the boxes, the radius is not read
struct GridGateArgs {
    int32_t S0, S1;
    GridSide a, b;
    GridOut out;
    int32_t* pairs; double* T_ref; int32_t* enable; int32_t* n_todo;
    bool sim_in, aabb;
};

struct SessionGateArgs {
    int32_t R;
    SessionTab tab;                                              // the tables on the device, and nb (host forms: only nb and has_gt, in host memory)
    const int32_t* sub_off; const int32_t* blocks; const int64_t* pair_off; const int64_t* tile_off;    // the tables in host memory: what is checked
    GridSide s;
    GridOut out;
    int32_t* pairs; double* T_ref; int32_t* enable; int32_t* todo_off;
    bool sim_in, aabb;
};

// The similarity is given: desc is not read, and `sim` stands where the gate would write it.  The cast is safe: k_grid_gate<true, .>
// and k_session_gate<true, .> only read out.sim, and a host form uploads it and never brings it back.
static void gate_sim_given(GridGateArgs& g, const double* sim) { g.sim_in = true; g.a.desc = g.b.desc = nullptr; g.out.sim = const_cast<double*>(sim); }
static void gate_sim_given(SessionGateArgs& g, const double* sim) { g.sim_in = true; g.s.desc = nullptr; g.out.sim = const_cast<double*>(sim); }

// --- pass 1 of the pair loop over a grid, radius mode ([REF roman/align/submap_align.py:93-149]) -------------------
static int grid_gate_check(roman_ctx* c, const roman_grid_gate_params_t* P, const GridGateArgs& g)
{
    { int rc = gate_params_check(c, P, g.sim_in, g.aabb, "roman_grid_gate_aabb*", g.S0 < 0 || g.S1 < 0, "S0 < 0 or S1 < 0"); if (rc) return rc; }
    if (!g.n_todo) return fail(c, ROMAN_E_INVALID, "n_todo is NULL");
    if (g.S0 == 0 || g.S1 == 0) return ROMAN_OK;
    if ((int64_t)g.S0 * g.S1 > (int64_t)(INT32_MAX / 16)) return fail(c, ROMAN_E_TOO_LARGE, "S0 * S1 = %lld pairs exceed the index width", (long long)g.S0 * g.S1);
    if (P->desc_dim > 0 && (!g.a.desc || !g.b.desc)) return fail(c, ROMAN_E_INVALID, "desc is NULL with desc_dim=%d", P->desc_dim);
    if (!g.a.pos || !g.b.pos || !g.a.T_w || !g.b.T_w) return fail(c, ROMAN_E_INVALID, "pos / T_w is NULL");
    if (g.aabb && (!g.a.box || !g.b.box)) return fail(c, ROMAN_E_INVALID, "box is NULL");
    if (P->single_robot_lc && (!g.a.time || !g.b.time)) return fail(c, ROMAN_E_INVALID, "time is NULL with single_robot_lc");
    if (!g.out.dist || !g.out.flags || !g.out.yaw_deg || !g.out.sim || !g.out.T_ij || !g.pairs || !g.T_ref || !g.enable) return fail(c, ROMAN_E_INVALID, "NULL output pointer");
    return ROMAN_OK;
}

// the device-pointer gate
static int grid_gate_dev(roman_ctx* c, const roman_grid_gate_params_t* gparams, const GridGateArgs& g)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = grid_gate_check(c, gparams, g);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    const int S0 = g.S0, S1 = g.S1;
    if (S0 == 0 || S1 == 0) { HIPCHK(c, hipMemsetAsync(g.n_todo, 0, sizeof(int32_t), stream)); return ROMAN_OK; }
    const int d = gparams->desc_dim, B = S0 * S1;
    HIPCHK(c, c->ggNorm.ensure(sizeof(double) * (size_t)(S0 + S1)));            // scratch first: a failure leaves nothing enqueued
    double* dNorm = c->ggNorm.as<double>();
    if (d > 0) hipLaunchKernelGGL(k_grid_norms, dim3((unsigned)((S0 + S1 + 3) / 4)), dim3(256), 0, stream, S0, S1, d, g.a.desc, g.b.desc, dNorm);
    const int64_t waves = (int64_t)S0 * ((S1 + GRID_TJ - 1) / GRID_TJ);
    hipLaunchKernelGGL(grid_gate_kernel(g.sim_in, g.aabb), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, *gparams, S0, S1, g.a, g.b, (const double*)dNorm, g.out);
    hipLaunchKernelGGL(k_grid_compact, dim3(1), dim3(B > 256 ? 1024 : 256), 0, stream, B, S1, (const int32_t*)g.out.flags, g.pairs, g.n_todo);
    hipLaunchKernelGGL(k_grid_fill, dim3((unsigned)(((int64_t)B * 16 + 255) / 256)), dim3(256), 0, stream, *gparams, S1, (const int32_t*)g.n_todo,
                       (const int32_t*)g.pairs, (const double*)g.out.T_ij, g.a.time, g.b.time, g.T_ref, g.enable);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// the host-pointer gate; sim_in: the caller's sim goes up and is not brought back
static int grid_gate_host(roman_ctx* c, const roman_grid_gate_params_t* gparams, const GridGateArgs& h)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = grid_gate_check(c, gparams, h);
    if (rc) return rc;
    if (h.S0 == 0 || h.S1 == 0) { *h.n_todo = 0; return ROMAN_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const size_t d = (size_t)gparams->desc_dim, S0 = (size_t)h.S0, S1 = (size_t)h.S1, B = S0 * S1;
    HostMirror m(c);
    const auto in = [&m](const double* p, size_t bytes) { return m.in(p, p ? bytes : 0); };          // an optional array that is absent stays absent
    const auto aPos = in(h.a.pos, 24 * S0), aGt = in(h.a.pos_gt, 24 * S0), aTw = in(h.a.T_w, 128 * S0), aTime = in(h.a.time, 8 * S0);
    const auto aDesc = in(h.a.desc, 8 * d * S0), aBox = in(h.a.box, 48 * S0);
    const auto bPos = in(h.b.pos, 24 * S1), bGt = in(h.b.pos_gt, 24 * S1), bTw = in(h.b.T_w, 128 * S1), bTime = in(h.b.time, 8 * S1);
    const auto bDesc = in(h.b.desc, 8 * d * S1), bBox = in(h.b.box, 48 * S1);
    const auto dDist = m.out(h.out.dist, 8 * B), dYaw = m.out(h.out.yaw_deg, 8 * B);
    const auto dSim = h.sim_in ? m.in(h.out.sim, 8 * B) : m.out(h.out.sim, 8 * B), dTij = m.out(h.out.T_ij, 128 * B);
    const auto dFlags = m.out(h.out.flags, 4 * B);
    // the compact outputs are inout: the slots beyond n_todo come back as they were
    const auto dTref = m.inout(h.T_ref, 128 * B);
    const auto dPairs = m.inout(h.pairs, 8 * B), dEn = m.inout(h.enable, 4 * B), dCnt = m.out(h.n_todo, 4);
    rc = m.upload();
    if (rc) return rc;
    GridGateArgs g = h;                                          // the same call on the mirror
    g.a.pos = aPos.dev(); g.a.pos_gt = aGt.dev(); g.a.T_w = aTw.dev(); g.a.time = aTime.dev(); g.a.desc = aDesc.dev(); g.a.box = aBox.dev();
    g.b.pos = bPos.dev(); g.b.pos_gt = bGt.dev(); g.b.T_w = bTw.dev(); g.b.time = bTime.dev(); g.b.desc = bDesc.dev(); g.b.box = bBox.dev();
    g.out.dist = dDist.dev(); g.out.flags = dFlags.dev(); g.out.yaw_deg = dYaw.dev(); g.out.sim = dSim.dev(); g.out.T_ij = dTij.dev();
    g.pairs = dPairs.dev(); g.T_ref = dTref.dev(); g.enable = dEn.dev(); g.n_todo = dCnt.dev();
    rc = grid_gate_dev(c, gparams, g);
    if (rc) return rc;
    return m.download();
}

int roman_grid_gate_dev(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                        const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                        const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                        double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                        int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo)
{
    GridGateArgs g{};
    g.S0 = S0; g.S1 = S1; g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.n_todo = n_todo;
    g.a.pos = pos0; g.a.pos_gt = pos_gt0; g.a.T_w = T_w0; g.a.time = time0; g.a.desc = desc0;
    g.b.pos = pos1; g.b.pos_gt = pos_gt1; g.b.T_w = T_w1; g.b.time = time1; g.b.desc = desc1;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    return grid_gate_dev(c, gparams, g);
}

int roman_grid_gate_sim_dev(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                            const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0,
                            const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1,
                            double* dist, int32_t* flags, double* yaw_deg, const double* sim, double* T_ij,
                            int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo)
{
    GridGateArgs g{};
    g.S0 = S0; g.S1 = S1; g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.n_todo = n_todo;
    g.a.pos = pos0; g.a.pos_gt = pos_gt0; g.a.T_w = T_w0; g.a.time = time0;
    g.b.pos = pos1; g.b.pos_gt = pos_gt1; g.b.T_w = T_w1; g.b.time = time1;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.T_ij = T_ij;
    gate_sim_given(g, sim);
    return grid_gate_dev(c, gparams, g);
}

// the AABB gate: NEARBY from the boxes roman_submap_boxes_dev wrote; with sim_in the similarity is an input
int roman_grid_gate_aabb_dev(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                             const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                             const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                             double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                             int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo,
                             const double* box0, const double* box1, const double* sim_in)
{
    GridGateArgs g{};
    g.S0 = S0; g.S1 = S1; g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.n_todo = n_todo; g.aabb = true;
    g.a.pos = pos0; g.a.pos_gt = pos_gt0; g.a.T_w = T_w0; g.a.time = time0; g.a.desc = desc0; g.a.box = box0;
    g.b.pos = pos1; g.b.pos_gt = pos_gt1; g.b.T_w = T_w1; g.b.time = time1; g.b.desc = desc1; g.b.box = box1;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    if (sim_in) gate_sim_given(g, sim_in);
    return grid_gate_dev(c, gparams, g);
}

int roman_grid_gate(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                    const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                    const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                    double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                    int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo)
{
    GridGateArgs g{};
    g.S0 = S0; g.S1 = S1; g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.n_todo = n_todo;
    g.a.pos = pos0; g.a.pos_gt = pos_gt0; g.a.T_w = T_w0; g.a.time = time0; g.a.desc = desc0;
    g.b.pos = pos1; g.b.pos_gt = pos_gt1; g.b.T_w = T_w1; g.b.time = time1; g.b.desc = desc1;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    return grid_gate_host(c, gparams, g);
}

int roman_grid_gate_sim(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                        const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0,
                        const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1,
                        double* dist, int32_t* flags, double* yaw_deg, const double* sim, double* T_ij,
                        int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo)
{
    GridGateArgs g{};
    g.S0 = S0; g.S1 = S1; g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.n_todo = n_todo;
    g.a.pos = pos0; g.a.pos_gt = pos_gt0; g.a.T_w = T_w0; g.a.time = time0;
    g.b.pos = pos1; g.b.pos_gt = pos_gt1; g.b.T_w = T_w1; g.b.time = time1;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.T_ij = T_ij;
    gate_sim_given(g, sim);
    return grid_gate_host(c, gparams, g);
}

int roman_grid_gate_aabb(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                         const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                         const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                         double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                         int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo,
                         const double* box0, const double* box1, const double* sim_in)
{
    GridGateArgs g{};
    g.S0 = S0; g.S1 = S1; g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.n_todo = n_todo; g.aabb = true;
    g.a.pos = pos0; g.a.pos_gt = pos_gt0; g.a.T_w = T_w0; g.a.time = time0; g.a.desc = desc0; g.a.box = box0;
    g.b.pos = pos1; g.b.pos_gt = pos_gt1; g.b.T_w = T_w1; g.b.time = time1; g.b.desc = desc1; g.b.box = box1;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    if (sim_in) gate_sim_given(g, sim_in);
    return grid_gate_host(c, gparams, g);
}

// --- pass 1 of a multi-robot session: the grids of a list of robot pairs in one launch sequence -------------------
// The tables are checked on their HOST copies (no read-back): -> *total = pair_off[nb], *tiles = tile_off[nb], *S = sub_off[R].
// sub_off, blocks and pair_off of a session (tile_off too where it is given), R >= 0, nb >= 0 and the pointers that are needed not NULL:
// -> *total = pair_off[nb], *tiles = the tiles of the gate, *self: a block sets self_lc
static int session_tables_check(roman_ctx* c, int32_t R, const int32_t* sub_off, int32_t nb, const int32_t* blocks, const int64_t* pair_off,
                                const int64_t* tile_off, int64_t* total, int64_t* tiles, bool* self_out)
{
    if (sub_off[0] != 0) return fail(c, ROMAN_E_INVALID, "sub_off[0] must be 0");
    for (int r = 0; r < R; ++r)
        if (sub_off[r + 1] < sub_off[r]) return fail(c, ROMAN_E_INVALID, "sub_off decreases at robot %d", r);
    bool self = false;
    int64_t po = 0, to = 0;
    std::vector<int64_t> seen;
    seen.reserve((size_t)nb);
    if (pair_off[0] != 0 || (tile_off && tile_off[0] != 0)) return fail(c, ROMAN_E_INVALID, "pair_off[0] and tile_off[0] must be 0");
    for (int b = 0; b < nb; ++b) {
        const int32_t r0 = blocks[4 * b], r1 = blocks[4 * b + 1];
        if (r0 < 0 || r0 >= R || r1 < 0 || r1 >= R) return fail(c, ROMAN_E_INVALID, "block %d names robot %d / %d outside [0, %d)", b, r0, r1, R);
        if (blocks[4 * b + 3] != 0) return fail(c, ROMAN_E_INVALID, "block %d: the reserved word must be 0", b);
        self = self || blocks[4 * b + 2] != 0;
        seen.push_back((int64_t)r0 * R + r1);
        const int64_t n0 = sub_off[r0 + 1] - sub_off[r0], n1 = sub_off[r1 + 1] - sub_off[r1];
        po += n0 * n1; to += n0 * ((n1 + GRID_TJ - 1) / GRID_TJ);
        if (po > (int64_t)(INT32_MAX / 16)) return fail(c, ROMAN_E_TOO_LARGE, "the blocks hold more than %d pairs: beyond the index width", INT32_MAX / 16);
        if (pair_off[b + 1] != po || (tile_off && tile_off[b + 1] != to)) return fail(c, ROMAN_E_INVALID, "pair_off / tile_off disagree with sub_off and blocks at block %d", b);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(c, ROMAN_E_INVALID, "a robot pair is listed twice");
    *total = po; *tiles = to; *self_out = self;
    return ROMAN_OK;
}

// the tables are judged on their host copies; what passes has pair_off[nb] pairs, tile_off[nb] tiles and sub_off[R] submaps
static int session_gate_check(roman_ctx* c, const roman_grid_gate_params_t* P, const SessionGateArgs& g)
{
    const int32_t R = g.R, nb = g.tab.nb;
    { int rc = gate_params_check(c, P, g.sim_in, g.aabb, "roman_session_gate_aabb*", R < 0 || nb < 0, "R < 0 or nb < 0"); if (rc) return rc; }
    if (!g.sub_off || !g.pair_off || !g.tile_off || !g.todo_off || (nb > 0 && !g.blocks)) return fail(c, ROMAN_E_INVALID, "sub_off / blocks / pair_off / tile_off / todo_off is NULL");
    bool self = false;
    int64_t total = 0, tiles = 0;
    { int rc = session_tables_check(c, R, g.sub_off, nb, g.blocks, g.pair_off, g.tile_off, &total, &tiles, &self); if (rc) return rc; }
    if (total == 0) return ROMAN_OK;
    if (P->desc_dim > 0 && !g.s.desc) return fail(c, ROMAN_E_INVALID, "desc is NULL with desc_dim=%d", P->desc_dim);
    if (!g.s.pos || !g.s.T_w) return fail(c, ROMAN_E_INVALID, "pos / T_w is NULL");
    if (g.aabb && !g.s.box) return fail(c, ROMAN_E_INVALID, "box is NULL");
    if (g.s.pos_gt && !g.tab.has_gt) return fail(c, ROMAN_E_INVALID, "has_gt is NULL with pos_gt");
    if (self && !g.s.time) return fail(c, ROMAN_E_INVALID, "time is NULL with a self_lc block");
    if (!g.out.dist || !g.out.flags || !g.out.yaw_deg || !g.out.sim || !g.out.T_ij || !g.pairs || !g.T_ref || !g.enable) return fail(c, ROMAN_E_INVALID, "NULL output pointer");
    return ROMAN_OK;
}

// the device-pointer session gate
static int session_gate_dev(roman_ctx* c, const roman_grid_gate_params_t* gparams, const SessionGateArgs& g)
{
    const SessionTab& tab = g.tab;
    // (the arguments are judged first — on host memory only, a NULL context included: fail() then keeps the text for roman_last_error(NULL))
    if (!tab.sub_off || !tab.pair_off || !tab.tile_off || (tab.nb > 0 && !tab.blocks)) return fail(c, ROMAN_E_INVALID, "a table is NULL on the device");
    int rc = session_gate_check(c, gparams, g);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    const int64_t total = g.pair_off[tab.nb], tiles = g.tile_off[tab.nb];
    const int S = g.sub_off[g.R];
    if (total == 0) { HIPCHK(c, hipMemsetAsync(g.todo_off, 0, sizeof(int32_t) * (size_t)(tab.nb + 1), stream)); return ROMAN_OK; }
    const int d = g.sim_in ? 0 : gparams->desc_dim;
    const int nwg = (int)((total + SESSION_SCAN - 1) / SESSION_SCAN);
    HIPCHK(c, c->ggNorm.ensure(sizeof(double) * (size_t)S));                    // scratch first: a failure leaves nothing enqueued
    HIPCHK(c, c->sgCount.ensure(sizeof(int32_t) * (size_t)nwg));
    double* dNorm = c->ggNorm.as<double>();
    int32_t* dCount = c->sgCount.as<int32_t>();
    if (d > 0) hipLaunchKernelGGL(k_grid_norms, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, stream, S, 0, d, g.s.desc, (const double*)nullptr, dNorm);
    hipLaunchKernelGGL(session_gate_kernel(g.sim_in, g.aabb), dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, *gparams, tab, tiles, g.s, (const double*)dNorm, g.out);
    hipLaunchKernelGGL(k_session_count, dim3((unsigned)nwg), dim3(SESSION_SCAN), 0, stream, total, (const int32_t*)g.out.flags, dCount);
    hipLaunchKernelGGL(k_session_scan, dim3(1), dim3(SESSION_SCAN), 0, stream, nwg, dCount, tab, total, g.todo_off);
    hipLaunchKernelGGL(k_session_scatter, dim3((unsigned)nwg), dim3(SESSION_SCAN), 0, stream, total, (const int32_t*)g.out.flags, (const int32_t*)dCount, tab, g.pairs, g.todo_off);
    hipLaunchKernelGGL(k_session_fill, dim3((unsigned)((total * 16 + 255) / 256)), dim3(256), 0, stream, *gparams, tab, (const int32_t*)g.todo_off,
                       (const int32_t*)g.pairs, (const double*)g.out.T_ij, g.s.time, g.T_ref, g.enable);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

// the host-pointer session gate; sim_in: the caller's `sim` goes up and is not brought back
static int session_gate_host(roman_ctx* c, const roman_grid_gate_params_t* gparams, const SessionGateArgs& h)
{
    int rc = session_gate_check(c, gparams, h);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const size_t R = (size_t)h.R, nb = (size_t)h.tab.nb, B = (size_t)h.pair_off[nb], nS = (size_t)h.sub_off[R];
    if (B == 0) { std::fill(h.todo_off, h.todo_off + nb + 1, 0); return ROMAN_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const size_t d = (size_t)gparams->desc_dim;
    HostMirror m(c);
    const auto dSub = m.in(h.sub_off, 4 * (R + 1)), dBlk = m.in(h.blocks, 16 * nb);
    const auto dPo = m.in(h.pair_off, 8 * (nb + 1)), dTo = m.in(h.tile_off, 8 * (nb + 1));
    const auto dPos = m.in(h.s.pos, 24 * nS), dGt = m.in(h.s.pos_gt, h.s.pos_gt ? 24 * nS : 0);
    const auto dHas = m.in(h.tab.has_gt, h.s.pos_gt ? 4 * R : 0);
    const auto dTw = m.in(h.s.T_w, 128 * nS), dTime = m.in(h.s.time, h.s.time ? 8 * nS : 0), dDesc = m.in(h.s.desc, h.s.desc ? 8 * d * nS : 0);
    const auto dBox = m.in(h.s.box, h.aabb ? 48 * nS : 0);
    const auto dDist = m.out(h.out.dist, 8 * B), dYaw = m.out(h.out.yaw_deg, 8 * B);
    const auto dSim = h.sim_in ? m.in(h.out.sim, 8 * B) : m.out(h.out.sim, 8 * B), dTij = m.out(h.out.T_ij, 128 * B);
    const auto dFlags = m.out(h.out.flags, 4 * B);
    // the compact outputs are inout: the slots beyond todo_off[nb] come back as they were
    const auto dTref = m.inout(h.T_ref, 128 * B);
    const auto dPairs = m.inout(h.pairs, 8 * B), dEn = m.inout(h.enable, 4 * B), dOff = m.out(h.todo_off, 4 * (nb + 1));
    rc = m.upload();
    if (rc) return rc;
    SessionGateArgs g = h;                                       // the same call on the mirror; the host tables stay the caller's
    g.tab.sub_off = dSub.dev(); g.tab.blocks = dBlk.dev(); g.tab.pair_off = dPo.dev(); g.tab.tile_off = dTo.dev(); g.tab.has_gt = dHas.dev();
    g.s.pos = dPos.dev(); g.s.pos_gt = dGt.dev(); g.s.T_w = dTw.dev(); g.s.time = dTime.dev(); g.s.desc = dDesc.dev(); g.s.box = dBox.dev();
    g.out.dist = dDist.dev(); g.out.flags = dFlags.dev(); g.out.yaw_deg = dYaw.dev(); g.out.sim = dSim.dev(); g.out.T_ij = dTij.dev();
    g.pairs = dPairs.dev(); g.T_ref = dTref.dev(); g.enable = dEn.dev(); g.todo_off = dOff.dev();
    rc = session_gate_dev(c, gparams, g);
    if (rc) return rc;
    return m.download();
}

int roman_session_gate_dev(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                           const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                           int32_t nb, const int32_t* blocks, const int32_t* blocks_host,
                           const int64_t* pair_off, const int64_t* pair_off_host, const int64_t* tile_off, const int64_t* tile_off_host,
                           double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                           int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off)
{
    SessionGateArgs g{};
    g.R = R; g.tab.nb = nb; g.tab.sub_off = sub_off; g.tab.blocks = blocks; g.tab.pair_off = pair_off; g.tab.tile_off = tile_off; g.tab.has_gt = has_gt;
    g.sub_off = sub_off_host; g.blocks = blocks_host; g.pair_off = pair_off_host; g.tile_off = tile_off_host;
    g.s.pos = pos; g.s.pos_gt = pos_gt; g.s.T_w = T_w; g.s.time = time; g.s.desc = desc;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.todo_off = todo_off;
    return session_gate_dev(c, gparams, g);
}

// `desc` is not read and `sim` is not written (both may be NULL): the similarity is sim_in
int roman_session_gate_sim_dev(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                               const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                               int32_t nb, const int32_t* blocks, const int32_t* blocks_host,
                               const int64_t* pair_off, const int64_t* pair_off_host, const int64_t* tile_off, const int64_t* tile_off_host,
                               double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                               int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* sim_in)
{
    (void)desc; (void)sim;
    SessionGateArgs g{};
    g.R = R; g.tab.nb = nb; g.tab.sub_off = sub_off; g.tab.blocks = blocks; g.tab.pair_off = pair_off; g.tab.tile_off = tile_off; g.tab.has_gt = has_gt;
    g.sub_off = sub_off_host; g.blocks = blocks_host; g.pair_off = pair_off_host; g.tile_off = tile_off_host;
    g.s.pos = pos; g.s.pos_gt = pos_gt; g.s.T_w = T_w; g.s.time = time;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.T_ij = T_ij;
    g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.todo_off = todo_off;
    gate_sim_given(g, sim_in);
    return session_gate_dev(c, gparams, g);
}

// the AABB gate of a session: NEARBY from the boxes roman_session_boxes_dev wrote; with sim_in the similarity is an
// input (`desc` is not read, `sim` not written), as roman_grid_gate_aabb* carries both
int roman_session_gate_aabb_dev(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                                const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                int32_t nb, const int32_t* blocks, const int32_t* blocks_host,
                                const int64_t* pair_off, const int64_t* pair_off_host, const int64_t* tile_off, const int64_t* tile_off_host,
                                double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* box, const double* sim_in)
{
    SessionGateArgs g{};
    g.R = R; g.tab.nb = nb; g.tab.sub_off = sub_off; g.tab.blocks = blocks; g.tab.pair_off = pair_off; g.tab.tile_off = tile_off; g.tab.has_gt = has_gt;
    g.sub_off = sub_off_host; g.blocks = blocks_host; g.pair_off = pair_off_host; g.tile_off = tile_off_host;
    g.s.pos = pos; g.s.pos_gt = pos_gt; g.s.T_w = T_w; g.s.time = time; g.s.desc = desc; g.s.box = box; g.aabb = true;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.todo_off = todo_off;
    if (sim_in) gate_sim_given(g, sim_in);
    return session_gate_dev(c, gparams, g);
}

int roman_session_gate(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                       const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                       int32_t nb, const int32_t* blocks, const int64_t* pair_off, const int64_t* tile_off,
                       double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                       int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off)
{
    SessionGateArgs g{};
    g.R = R; g.tab.nb = nb; g.tab.has_gt = has_gt; g.sub_off = sub_off; g.blocks = blocks; g.pair_off = pair_off; g.tile_off = tile_off;
    g.s.pos = pos; g.s.pos_gt = pos_gt; g.s.T_w = T_w; g.s.time = time; g.s.desc = desc;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.todo_off = todo_off;
    return session_gate_host(c, gparams, g);
}

int roman_session_gate_sim(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                           const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                           int32_t nb, const int32_t* blocks, const int64_t* pair_off, const int64_t* tile_off,
                           double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                           int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* sim_in)
{
    (void)desc; (void)sim;
    SessionGateArgs g{};
    g.R = R; g.tab.nb = nb; g.tab.has_gt = has_gt; g.sub_off = sub_off; g.blocks = blocks; g.pair_off = pair_off; g.tile_off = tile_off;
    g.s.pos = pos; g.s.pos_gt = pos_gt; g.s.T_w = T_w; g.s.time = time;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.T_ij = T_ij;
    g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.todo_off = todo_off;
    gate_sim_given(g, sim_in);
    return session_gate_host(c, gparams, g);
}

int roman_session_gate_aabb(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                            const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                            int32_t nb, const int32_t* blocks, const int64_t* pair_off, const int64_t* tile_off,
                            double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                            int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* box, const double* sim_in)
{
    SessionGateArgs g{};
    g.R = R; g.tab.nb = nb; g.tab.has_gt = has_gt; g.sub_off = sub_off; g.blocks = blocks; g.pair_off = pair_off; g.tile_off = tile_off;
    g.s.pos = pos; g.s.pos_gt = pos_gt; g.s.T_w = T_w; g.s.time = time; g.s.desc = desc; g.s.box = box; g.aabb = true;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.todo_off = todo_off;
    if (sim_in) gate_sim_given(g, sim_in);
    return session_gate_host(c, gparams, g);
}

// --- pass 1 of a session over an explicit pair list ---------------------------------------------------------------
// SessionGateArgs as the whole-grid calls fill them (no tile_off: the list is the work), and the list: on the device (host forms:
// NULL), in host memory (what is checked), and the similarity of every pair of every block where it is given.
struct SessionListArgs {
    SessionGateArgs g;
    int32_t L; const int32_t* list; const int32_t* list_host;
    const double* sim_in;
};

static auto session_gate_list_kernel(bool sim_in, bool aabb)
{
    return sim_in ? (aabb ? k_session_gate_list<true, true> : k_session_gate_list<true, false>)
                  : (aabb ? k_session_gate_list<false, true> : k_session_gate_list<false, false>);
}

// A pair list (L > 0 entries (b, i, j)) on its host copy, against tables that passed session_tables_check — what
// roman_session_gate_list* and roman_session_stacked_sim_list* refuse about it
static int session_pair_list_check(roman_ctx* c, const int32_t* sub_off, int32_t nb, const int32_t* blocks, int32_t L, const int32_t* list_host)
{
    if ((int64_t)L > (int64_t)(INT32_MAX / 16)) return fail(c, ROMAN_E_TOO_LARGE, "L = %d pairs: L * 16 exceeds the index width", L);
    if (!list_host) return fail(c, ROMAN_E_INVALID, "list is NULL with L=%d", L);
    for (int64_t l = 0; l < L; ++l) {
        const int32_t* e = list_host + 3 * l;
        if (e[0] < 0 || e[0] >= nb) return fail(c, ROMAN_E_INVALID, "list entry %lld names block %d outside [0, %d)", (long long)l, e[0], nb);
        const int32_t r0 = blocks[4 * e[0]], r1 = blocks[4 * e[0] + 1];
        const int32_t n0 = sub_off[r0 + 1] - sub_off[r0], n1 = sub_off[r1 + 1] - sub_off[r1];
        if (e[1] < 0 || e[1] >= n0 || e[2] < 0 || e[2] >= n1)
            return fail(c, ROMAN_E_INVALID, "list entry %lld: pair (%d, %d) lies outside the %d x %d grid of block %d", (long long)l, e[1], e[2], n0, n1, e[0]);
        if (l > 0 && !std::lexicographical_compare(e - 3, e, e, e + 3))
            return fail(c, ROMAN_E_INVALID, "the list is not strictly ascending in (block, i, j) at entry %lld", (long long)l);
    }
    return ROMAN_OK;
}

// the tables first (session_tables_check, as the whole-grid calls judge them), then the list on its host copy
static int session_gate_list_check(roman_ctx* c, const roman_grid_gate_params_t* P, const SessionListArgs& a)
{
    const SessionGateArgs& g = a.g;
    const int32_t R = g.R, nb = g.tab.nb, L = a.L;
    { int rc = gate_params_check(c, P, g.sim_in, g.aabb, "roman_session_gate_list* with box", R < 0 || nb < 0 || L < 0, "R < 0, nb < 0 or L < 0"); if (rc) return rc; }
    if (!g.sub_off || !g.pair_off || !g.todo_off || (nb > 0 && !g.blocks)) return fail(c, ROMAN_E_INVALID, "sub_off / blocks / pair_off / todo_off is NULL");
    bool self = false;
    int64_t total = 0, tiles = 0;
    { int rc = session_tables_check(c, R, g.sub_off, nb, g.blocks, g.pair_off, nullptr, &total, &tiles, &self); if (rc) return rc; }
    if (L == 0) return ROMAN_OK;
    { int rc = session_pair_list_check(c, g.sub_off, nb, g.blocks, L, a.list_host); if (rc) return rc; }
    if (P->desc_dim > 0 && !g.s.desc) return fail(c, ROMAN_E_INVALID, "desc is NULL with desc_dim=%d", P->desc_dim);
    if (!g.s.pos || !g.s.T_w) return fail(c, ROMAN_E_INVALID, "pos / T_w is NULL");
    if (g.s.pos_gt && !g.tab.has_gt) return fail(c, ROMAN_E_INVALID, "has_gt is NULL with pos_gt");
    if (self && !g.s.time) return fail(c, ROMAN_E_INVALID, "time is NULL with a self_lc block");
    if (!g.out.dist || !g.out.flags || !g.out.yaw_deg || !g.out.sim || !g.out.T_ij || !g.pairs || !g.T_ref || !g.enable) return fail(c, ROMAN_E_INVALID, "NULL output pointer");
    return ROMAN_OK;
}

// the device-pointer list gate
static int session_gate_list_dev(roman_ctx* c, const roman_grid_gate_params_t* gparams, const SessionListArgs& a)
{
    const SessionGateArgs& g = a.g;
    const SessionTab& tab = g.tab;
    // (the arguments are judged first — on host memory only, a NULL context included)
    if (!tab.sub_off || !tab.pair_off || (tab.nb > 0 && !tab.blocks) || (a.L > 0 && !a.list)) return fail(c, ROMAN_E_INVALID, "a table or the list is NULL on the device");
    int rc = session_gate_list_check(c, gparams, a);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    const int L = a.L, S = g.sub_off[g.R];
    if (L == 0) { HIPCHK(c, hipMemsetAsync(g.todo_off, 0, sizeof(int32_t) * (size_t)(tab.nb + 1), stream)); return ROMAN_OK; }
    const int d = g.sim_in ? 0 : gparams->desc_dim;
    const int nwg = (L + SESSION_SCAN - 1) / SESSION_SCAN;
    HIPCHK(c, c->ggNorm.ensure(sizeof(double) * (size_t)S));                    // scratch first: a failure leaves nothing enqueued
    HIPCHK(c, c->sgCount.ensure(sizeof(int32_t) * ((size_t)nwg + (size_t)L)));  // the workgroup counts, then the source entry of every compact slot
    double* dNorm = c->ggNorm.as<double>();
    int32_t* dCount = c->sgCount.as<int32_t>();
    int32_t* dSrc = dCount + nwg;
    const int waves = (L + GRID_TJ - 1) / GRID_TJ;
    if (d > 0) hipLaunchKernelGGL(k_grid_norms, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, stream, S, 0, d, g.s.desc, (const double*)nullptr, dNorm);
    hipLaunchKernelGGL(session_gate_list_kernel(g.sim_in, g.aabb), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, *gparams, tab, L, a.list, g.s,
                       (const double*)dNorm, a.sim_in, g.out);
    hipLaunchKernelGGL(k_session_count, dim3((unsigned)nwg), dim3(SESSION_SCAN), 0, stream, (int64_t)L, (const int32_t*)g.out.flags, dCount);
    hipLaunchKernelGGL(k_session_list_scan, dim3(1), dim3(SESSION_SCAN), 0, stream, nwg, dCount, tab.nb, L, a.list, g.todo_off);
    hipLaunchKernelGGL(k_session_list_scatter, dim3((unsigned)nwg), dim3(SESSION_SCAN), 0, stream, L, (const int32_t*)g.out.flags, (const int32_t*)dCount, tab, a.list,
                       g.pairs, dSrc, g.todo_off);
    hipLaunchKernelGGL(k_session_list_fill, dim3((unsigned)(((int64_t)L * 16 + 255) / 256)), dim3(256), 0, stream, *gparams, tab, (const int32_t*)g.todo_off,
                       (const int32_t*)g.pairs, (const int32_t*)dSrc, a.list, (const double*)g.out.T_ij, g.s.time, g.T_ref, g.enable);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_session_gate_list_dev(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                                const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                int32_t nb, const int32_t* blocks, const int32_t* blocks_host, const int64_t* pair_off, const int64_t* pair_off_host,
                                int32_t L, const int32_t* list, const int32_t* list_host, const double* box, const double* sim_in,
                                double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off)
{
    SessionListArgs a{};
    SessionGateArgs& g = a.g;
    g.R = R; g.tab.nb = nb; g.tab.sub_off = sub_off; g.tab.blocks = blocks; g.tab.pair_off = pair_off; g.tab.has_gt = has_gt;
    g.sub_off = sub_off_host; g.blocks = blocks_host; g.pair_off = pair_off_host;
    g.s.pos = pos; g.s.pos_gt = pos_gt; g.s.T_w = T_w; g.s.time = time; g.s.desc = sim_in ? nullptr : desc; g.s.box = box; g.aabb = box != nullptr;
    g.out.dist = dist; g.out.flags = flags; g.out.yaw_deg = yaw_deg; g.out.sim = sim; g.out.T_ij = T_ij;
    g.pairs = pairs; g.T_ref = T_ref; g.enable = enable; g.todo_off = todo_off; g.sim_in = sim_in != nullptr;
    a.L = L; a.list = list; a.list_host = list_host; a.sim_in = sim_in;
    return session_gate_list_dev(c, gparams, a);
}

// the host-pointer list gate: everything goes up, sim_in included, and every output comes back with one synchronisation
int roman_session_gate_list(roman_ctx_t* c, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                            const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                            int32_t nb, const int32_t* blocks, const int64_t* pair_off, int32_t L, const int32_t* list, const double* box, const double* sim_in,
                            double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                            int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off)
{
    SessionListArgs h{};
    h.g.R = R; h.g.tab.nb = nb; h.g.tab.has_gt = has_gt; h.g.sub_off = sub_off; h.g.blocks = blocks; h.g.pair_off = pair_off;
    h.g.s.pos = pos; h.g.s.pos_gt = pos_gt; h.g.s.T_w = T_w; h.g.s.time = time; h.g.s.desc = sim_in ? nullptr : desc; h.g.s.box = box; h.g.aabb = box != nullptr;
    h.g.out.dist = dist; h.g.out.flags = flags; h.g.out.yaw_deg = yaw_deg; h.g.out.sim = sim; h.g.out.T_ij = T_ij;
    h.g.pairs = pairs; h.g.T_ref = T_ref; h.g.enable = enable; h.g.todo_off = todo_off; h.g.sim_in = sim_in != nullptr;
    h.L = L; h.list_host = list; h.sim_in = sim_in;
    int rc = session_gate_list_check(c, gparams, h);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const size_t nR = (size_t)R, nB = (size_t)nb, B = (size_t)pair_off[nb], nS = (size_t)sub_off[R], nL = (size_t)L;
    if (L == 0) { std::fill(todo_off, todo_off + nB + 1, 0); return ROMAN_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const size_t d = sim_in ? 0 : (size_t)gparams->desc_dim;
    HostMirror m(c);
    const auto dSub = m.in(sub_off, 4 * (nR + 1)), dBlk = m.in(blocks, 16 * nB), dList = m.in(list, 12 * nL);
    const auto dPo = m.in(pair_off, 8 * (nB + 1));
    const auto dPos = m.in(pos, 24 * nS), dGt = m.in(pos_gt, pos_gt ? 24 * nS : 0);
    const auto dHas = m.in(has_gt, pos_gt ? 4 * nR : 0);
    const auto dTw = m.in(T_w, 128 * nS), dTime = m.in(time, time ? 8 * nS : 0), dDesc = m.in(h.g.s.desc, h.g.s.desc ? 8 * d * nS : 0);
    const auto dBox = m.in(box, box ? 48 * nS : 0), dSin = m.in(sim_in, sim_in ? 8 * B : 0);
    const auto dDist = m.out(dist, 8 * nL), dYaw = m.out(yaw_deg, 8 * nL), dSim = m.out(sim, 8 * nL), dTij = m.out(T_ij, 128 * nL);
    const auto dFlags = m.out(flags, 4 * nL);
    // the compact outputs are inout: the slots beyond todo_off[nb] come back as they were
    const auto dTref = m.inout(T_ref, 128 * nL);
    const auto dPairs = m.inout(pairs, 8 * nL), dEn = m.inout(enable, 4 * nL), dOff = m.out(todo_off, 4 * (nB + 1));
    rc = m.upload();
    if (rc) return rc;
    SessionListArgs a = h;                                       // the same call on the mirror; the host tables stay the caller's
    SessionGateArgs& g = a.g;
    g.tab.sub_off = dSub.dev(); g.tab.blocks = dBlk.dev(); g.tab.pair_off = dPo.dev(); g.tab.has_gt = dHas.dev();
    g.s.pos = dPos.dev(); g.s.pos_gt = dGt.dev(); g.s.T_w = dTw.dev(); g.s.time = dTime.dev(); g.s.desc = dDesc.dev(); g.s.box = dBox.dev();
    g.out.dist = dDist.dev(); g.out.flags = dFlags.dev(); g.out.yaw_deg = dYaw.dev(); g.out.sim = dSim.dev(); g.out.T_ij = dTij.dev();
    g.pairs = dPairs.dev(); g.T_ref = dTref.dev(); g.enable = dEn.dev(); g.todo_off = dOff.dev();
    a.list = dList.dev(); a.sim_in = dSin.dev();
    rc = session_gate_list_dev(c, gparams, a);
    if (rc) return rc;
    return m.download();
}

// --- frame descriptors of the submaps of a pool ([REF roman/map/map.py:210-242], [REF :155-162]) ------------------
static int frame_select_check(roman_ctx* c, const roman_frame_select_params_t* P, int32_t S, int32_t cap, const void* count, const void* src,
                              int32_t N, const void* seg_times, int32_t Nf, const void* frame_times, const void* frame_pos, int32_t d,
                              const void* frame_desc, const void* mask, const void* n_sel, const void* span, const void* mean)
{
    if (!P) return fail(c, ROMAN_E_INVALID, "fparams is NULL");
    if (S < 0 || N < 0 || Nf < 0 || d < 0) return fail(c, ROMAN_E_INVALID, "S, N, Nf or d is negative");
    if (cap < 1) return fail(c, ROMAN_E_INVALID, "cap must be >= 1 (got %d)", cap);
    if (P->reserved[0] != 0 || P->reserved[1] != 0) return fail(c, ROMAN_E_INVALID, "roman_frame_select_params_t reserved words must be 0");
    if (P->thin && (P->thin_dist != P->thin_dist || P->thin_dist < 0.0)) return fail(c, ROMAN_E_INVALID, "thin_dist=%g must be a distance >= 0", P->thin_dist);
    if (P->want_mean && (d < 1 || (Nf > 0 && !frame_desc))) return fail(c, ROMAN_E_INVALID, "want_mean needs d >= 1 and frame_desc");
    if ((int64_t)S * cap > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "S * cap = %lld rows exceed the index width", (long long)S * cap);
    if (S == 0) return ROMAN_OK;
    if (!count || !src || !n_sel || !span || (Nf > 0 && !mask) || (P->want_mean && !mean)) return fail(c, ROMAN_E_INVALID, "NULL count, src or output pointer");
    if (N > 0 && !seg_times) return fail(c, ROMAN_E_INVALID, "seg_times is NULL");
    if (Nf > 0 && (!frame_times || (P->thin && !frame_pos))) return fail(c, ROMAN_E_INVALID, "frame_times / frame_pos is NULL");
    return ROMAN_OK;
}

int roman_frame_select_dev(roman_ctx_t* c, const roman_frame_select_params_t* fparams, int32_t S, int32_t cap,
                           const int32_t* count, const int32_t* src, int32_t N, const double* seg_times,
                           int32_t Nf, const double* frame_times, const double* frame_pos, int32_t d, const double* frame_desc,
                           uint64_t* mask, int32_t* n_sel, double* span, double* mean)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = frame_select_check(c, fparams, S, cap, count, src, N, seg_times, Nf, frame_times, frame_pos, d, frame_desc, mask, n_sel, span, mean);
    if (rc || S == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    hipLaunchKernelGGL(k_frame_select, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, stream, *fparams, (int)S, (int)cap, count, src, (int)N, seg_times,
                       (int)Nf, frame_times, frame_pos, reinterpret_cast<unsigned long long*>(mask), n_sel, span);
    if (fparams->want_mean)
        hipLaunchKernelGGL(k_frame_mean, dim3((unsigned)S, (unsigned)((d + 255) / 256)), dim3(256), 0, stream, (int)Nf, (int)d, frame_desc,
                           reinterpret_cast<const unsigned long long*>(mask), (const int32_t*)n_sel, mean);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_frame_select(roman_ctx_t* c, const roman_frame_select_params_t* fparams, int32_t S, int32_t cap,
                       const int32_t* count, const int32_t* src, int32_t N, const double* seg_times,
                       int32_t Nf, const double* frame_times, const double* frame_pos, int32_t d, const double* frame_desc,
                       uint64_t* mask, int32_t* n_sel, double* span, double* mean)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = frame_select_check(c, fparams, S, cap, count, src, N, seg_times, Nf, frame_times, frame_pos, d, frame_desc, mask, n_sel, span, mean);
    if (rc || S == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const bool thin = fparams->thin != 0, wm = fparams->want_mean != 0;
    const size_t W = ((size_t)Nf + 63) / 64;
    HostMirror m(c);
    const auto cnt = m.in(count, 4 * (size_t)S);
    const auto dSrc = m.in(src, 4 * (size_t)S * (size_t)cap);
    const auto seg = m.in(seg_times, 16 * (size_t)N);
    const auto ft = m.in(frame_times, 8 * (size_t)Nf);
    const auto fp = m.in(frame_pos, thin ? 24 * (size_t)Nf : 0);
    const auto fd = m.in(frame_desc, wm ? 8 * (size_t)Nf * (size_t)d : 0);
    const auto dMask = m.out(mask, 8 * (size_t)S * W);
    const auto sel = m.out(n_sel, 4 * (size_t)S);
    const auto dSpan = m.out(span, 16 * (size_t)S);
    const auto dMean = m.out(mean, wm ? 8 * (size_t)S * (size_t)d : 0);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_frame_select_dev(c, fparams, S, cap, cnt.dev(), dSrc.dev(), N, seg.dev(), Nf, ft.dev(), fp.dev(), d, fd.dev(),
                                dMask.dev(), sel.dev(), dSpan.dev(), dMean.dev());
    if (rc) return rc;
    return m.download();
}

// --- the LISTED slots of a session whose frame tables stay in HBM ---------------------------------------------------
// What one call works on, under names; the host form hands the device form a copy whose bulk arrays are the mirror's.  robots and list
// are HOST memory in both forms.
struct SessionFrameArgs {
    int32_t R; const roman_session_frame_robot_t* robots; int32_t cap;
    const int32_t* count; const int32_t* src; const double* seg_times; const double* frame_times; const double* frame_pos;
    int32_t d; const double* frame_desc; int32_t L; const int32_t* list;
    uint64_t* mask; int32_t* n_sel; double* span; double* mean; int32_t* changed;
};
// the extents the robots' ranges span: segment rows, slots, frames, mask words
struct SessionFrameExtent { int64_t seg = 0, sub = 0, frames = 0, words = 0; };

// the header's order: the parameter block (frame_select_check's own), the robots, the list, the sizes, the pointers
static int session_frame_check(roman_ctx* c, const roman_frame_select_params_t* P, const SessionFrameArgs& g, SessionFrameExtent* x)
{
    int rc = frame_select_check(c, P, 0, g.cap, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, g.d, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (g.R < 0) return fail(c, ROMAN_E_INVALID, "R < 0");
    if (g.R > 0 && !g.robots) return fail(c, ROMAN_E_INVALID, "robots is NULL");
    SessionFrameExtent e;
    for (int r = 0; r < g.R; ++r) {
        const roman_session_frame_robot_t& b = g.robots[r];
        if (b.reserved[0] != 0 || b.reserved[1] != 0) return fail(c, ROMAN_E_INVALID, "roman_session_frame_robot_t reserved words must be 0 (robot %d)", r);
        if (b.seg0 < 0 || b.mask_off < 0 || b.n_seg < 0 || b.sub0 < 0 || b.n_sub < 0 || b.frame0 < 0 || b.n_frames < 0 || b.mask_words < 0)
            return fail(c, ROMAN_E_INVALID, "robot %d holds a negative size or offset", r);
        if ((int64_t)b.mask_words < ((int64_t)b.n_frames + 63) / 64)
            return fail(c, ROMAN_E_INVALID, "robot %d: mask_words=%d is less than the %lld words of its %d frames", r, b.mask_words,
                        (long long)(((int64_t)b.n_frames + 63) / 64), b.n_frames);
        if (b.seg0 < e.seg || b.sub0 < e.sub || b.frame0 < e.frames || b.mask_off < e.words)
            return fail(c, ROMAN_E_INVALID, "the ranges of robot %d are not ascending and disjoint", r);
        e.seg = b.seg0 + b.n_seg; e.sub = (int64_t)b.sub0 + b.n_sub; e.frames = (int64_t)b.frame0 + b.n_frames;
        e.words = b.mask_off + (int64_t)b.n_sub * b.mask_words;
    }
    if (g.L < 0) return fail(c, ROMAN_E_INVALID, "L < 0");
    if (g.L > 0 && !g.list) return fail(c, ROMAN_E_INVALID, "list is NULL");
    for (int32_t l = 0, r = 0; l < g.L; ++l) {
        const int32_t s = g.list[l];
        if (s < 0 || s >= e.sub) return fail(c, ROMAN_E_INVALID, "list[%d] = %d outside the %lld slots of the session", l, s, (long long)e.sub);
        if (l > 0 && s <= g.list[l - 1]) return fail(c, ROMAN_E_INVALID, "list is not strictly ascending at entry %d", l);
        while ((int64_t)s >= (int64_t)g.robots[r].sub0 + g.robots[r].n_sub) ++r;                 // (s < e.sub: a robot ends behind it)
        if (s < g.robots[r].sub0) return fail(c, ROMAN_E_INVALID, "list[%d] = %d lies between the slots of two robots", l, s);
    }
    if (e.sub > (int64_t)INT32_MAX || e.frames > (int64_t)INT32_MAX || e.sub * g.cap > (int64_t)INT32_MAX)
        return fail(c, ROMAN_E_TOO_LARGE, "%lld slots of %d rows or %lld frames exceed the index width", (long long)e.sub, g.cap, (long long)e.frames);
    *x = e;
    if (g.L == 0) return ROMAN_OK;
    if (!g.count || !g.src || !g.n_sel || !g.span || !g.changed || (e.words > 0 && !g.mask) || (P->want_mean && !g.mean))
        return fail(c, ROMAN_E_INVALID, "NULL count, src or output pointer");
    if (e.seg > 0 && !g.seg_times) return fail(c, ROMAN_E_INVALID, "seg_times is NULL");
    if (e.frames > 0 && (!g.frame_times || (P->thin && !g.frame_pos) || (P->want_mean && !g.frame_desc)))
        return fail(c, ROMAN_E_INVALID, "frame_times / frame_pos / frame_desc is NULL");
    return ROMAN_OK;
}

static int session_frame_select_list_dev(roman_ctx* c, const roman_frame_select_params_t* fparams, const SessionFrameArgs& g)
{
    SessionFrameExtent x;
    int rc = session_frame_check(c, fparams, g, &x);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (g.L == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    // the robots' records and the list behind them as ONE staged block of 64-bit words: a pure enqueue
    constexpr size_t RW = sizeof(SessionFrameRobot) / sizeof(int64_t);
    const size_t words = RW * (size_t)g.R + ((size_t)g.L + 1) / 2;
    int64_t* staged = nullptr;
    HIPCHK(c, c->sfTab.ensure(sizeof(int64_t) * words));
    HIPCHK(c, c->sfStage.stage(words, &staged));
    memcpy(staged, g.robots, sizeof(SessionFrameRobot) * (size_t)g.R);
    staged[words - 1] = 0;
    memcpy(staged + RW * (size_t)g.R, g.list, sizeof(int32_t) * (size_t)g.L);
    HIPCHK(c, c->sfStage.upload(c->sfTab, words, stream));
    const SessionFrameRobot* dRobots = c->sfTab.as<SessionFrameRobot>();
    const int32_t* dList = reinterpret_cast<const int32_t*>(c->sfTab.as<int64_t>() + RW * (size_t)g.R);
    hipLaunchKernelGGL(k_session_frame_select_list, dim3((unsigned)((g.L + 3) / 4)), dim3(256), 0, stream, *fparams, (int)g.L, (int)g.R, dList, dRobots, (int)g.cap,
                       g.count, g.src, g.seg_times, g.frame_times, g.frame_pos, reinterpret_cast<unsigned long long*>(g.mask), g.n_sel, g.span, g.changed);
    if (fparams->want_mean)
        hipLaunchKernelGGL(k_session_frame_mean_list, dim3((unsigned)g.L, (unsigned)((g.d + 255) / 256)), dim3(256), 0, stream, (int)g.R, dList, dRobots, (int)g.d,
                           g.frame_desc, reinterpret_cast<const unsigned long long*>(g.mask), (const int32_t*)g.n_sel, g.mean, g.changed);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

static int session_frame_select_list_host(roman_ctx* c, const roman_frame_select_params_t* fparams, const SessionFrameArgs& h)
{
    SessionFrameExtent x;
    int rc = session_frame_check(c, fparams, h, &x);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (h.L == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const bool thin = fparams->thin != 0, wm = fparams->want_mean != 0;
    HostMirror m(c);
    const auto cnt = m.in(h.count, 4 * (size_t)x.sub);
    const auto dSrc = m.in(h.src, 4 * (size_t)x.sub * (size_t)h.cap);
    const auto seg = m.in(h.seg_times, 16 * (size_t)x.seg);
    const auto ft = m.in(h.frame_times, 8 * (size_t)x.frames);
    const auto fp = m.in(h.frame_pos, thin ? 24 * (size_t)x.frames : 0);
    const auto fd = m.in(h.frame_desc, wm ? 8 * (size_t)x.frames * (size_t)h.d : 0);
    const auto dMask = m.inout(h.mask, 8 * (size_t)x.words);
    const auto sel = m.inout(h.n_sel, 4 * (size_t)x.sub);
    const auto dSpan = m.inout(h.span, 16 * (size_t)x.sub);
    const auto dMean = m.inout(h.mean, wm ? 8 * (size_t)x.sub * (size_t)h.d : 0);
    const auto chg = m.out(h.changed, 4 * (size_t)h.L);
    rc = m.upload();
    if (rc) return rc;
    SessionFrameArgs g = h;
    g.count = cnt.dev(); g.src = dSrc.dev(); g.seg_times = seg.dev(); g.frame_times = ft.dev(); g.frame_pos = fp.dev(); g.frame_desc = fd.dev();
    g.mask = dMask.dev(); g.n_sel = sel.dev(); g.span = dSpan.dev(); g.mean = dMean.dev(); g.changed = chg.dev();
    rc = session_frame_select_list_dev(c, fparams, g);
    if (rc) return rc;
    return m.download();
}

int roman_session_frame_select_list_dev(roman_ctx_t* c, const roman_frame_select_params_t* fparams, int32_t R, const roman_session_frame_robot_t* robots,
                                        int32_t cap, const int32_t* count, const int32_t* src, const double* seg_times, const double* frame_times,
                                        const double* frame_pos, int32_t d, const double* frame_desc, int32_t L, const int32_t* list,
                                        uint64_t* mask, int32_t* n_sel, double* span, double* mean, int32_t* changed)
{
    const SessionFrameArgs g{R, robots, cap, count, src, seg_times, frame_times, frame_pos, d, frame_desc, L, list, mask, n_sel, span, mean, changed};
    return session_frame_select_list_dev(c, fparams, g);
}

int roman_session_frame_select_list(roman_ctx_t* c, const roman_frame_select_params_t* fparams, int32_t R, const roman_session_frame_robot_t* robots,
                                    int32_t cap, const int32_t* count, const int32_t* src, const double* seg_times, const double* frame_times,
                                    const double* frame_pos, int32_t d, const double* frame_desc, int32_t L, const int32_t* list,
                                    uint64_t* mask, int32_t* n_sel, double* span, double* mean, int32_t* changed)
{
    const SessionFrameArgs g{R, robots, cap, count, src, seg_times, frame_times, frame_pos, d, frame_desc, L, list, mask, n_sel, span, mean, changed};
    return session_frame_select_list_host(c, fparams, g);
}

static int stacked_sim_check(roman_ctx* c, int32_t d, int32_t Nf0, const void* desc0, int32_t S0, const void* mask0,
                             int32_t Nf1, const void* desc1, int32_t S1, const void* mask1, const void* sim)
{
    if (d < 1) return fail(c, ROMAN_E_INVALID, "d=%d: a frame descriptor has at least one component", d);
    if (Nf0 < 0 || Nf1 < 0 || S0 < 0 || S1 < 0) return fail(c, ROMAN_E_INVALID, "a size is negative");
    if ((int64_t)S0 * S1 > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "S0 * S1 = %lld pairs exceed the index width", (long long)S0 * S1);
    if (S0 == 0 || S1 == 0) return ROMAN_OK;
    if (!sim) return fail(c, ROMAN_E_INVALID, "sim is NULL");
    if ((Nf0 > 0 && (!desc0 || !mask0)) || (Nf1 > 0 && (!desc1 || !mask1))) return fail(c, ROMAN_E_INVALID, "desc / mask is NULL");
    if (((int64_t)S0 * (((int64_t)Nf1 + 255) / 256)) > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "S0 * Nf1 exceeds the launch width");
    return ROMAN_OK;
}

int roman_ctx_set_stacked_band(roman_ctx_t* c, int32_t rows)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (rows < 0) return fail(c, ROMAN_E_INVALID, "rows=%d is negative", rows);
    c->stacked_band = rows == 0 ? 0 : (int)std::min<int64_t>((((int64_t)rows + STACK_TILE - 1) / STACK_TILE) * STACK_TILE, INT32_MAX / STACK_TILE * STACK_TILE);
    return ROMAN_OK;
}

int roman_stacked_sim_dev(roman_ctx_t* c, int32_t d, int32_t Nf0, const double* desc0, int32_t S0, const uint64_t* mask0,
                          int32_t Nf1, const double* desc1, int32_t S1, const uint64_t* mask1, double* sim)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = stacked_sim_check(c, d, Nf0, desc0, S0, mask0, Nf1, desc1, S1, mask1, sim);
    if (rc || S0 == 0 || S1 == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    const int64_t B = (int64_t)S0 * S1;
    if (Nf0 == 0 || Nf1 == 0) {                                  // no frame pair: the maximum over nothing
        hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, -(double)INFINITY, sim);
        HIPCHK(c, hipGetLastError());
        return ROMAN_OK;
    }
    // rows of a band: what was set, or what 64 MiB hold; a multiple of STACK_TILE, at most the frames there are
    const int64_t rounded = (((int64_t)Nf0 + STACK_TILE - 1) / STACK_TILE) * STACK_TILE;
    int64_t H = c->stacked_band > 0 ? c->stacked_band : std::max<int64_t>(STACK_TILE, ((int64_t)(64 << 20) / 8 / Nf1) / STACK_TILE * STACK_TILE);
    H = std::min(H, rounded);
    // scratch first: a failure leaves nothing enqueued
    HIPCHK(c, c->ssNorm.ensure(sizeof(double) * ((size_t)Nf0 + (size_t)Nf1)));
    HIPCHK(c, c->ssBand.ensure(sizeof(double) * (size_t)std::min<int64_t>(H, Nf0) * (size_t)Nf1));
    HIPCHK(c, c->ssR.ensure(sizeof(double) * (size_t)S0 * (size_t)Nf1));
    double* const dNorm = c->ssNorm.as<double>();
    double* const Cb = c->ssBand.as<double>();
    double* const R = c->ssR.as<double>();
    const int W0 = (Nf0 + 63) / 64, W1 = (Nf1 + 63) / 64, nbx = (Nf1 + 255) / 256;
    hipLaunchKernelGGL(k_grid_norms, dim3((unsigned)(((int64_t)Nf0 + Nf1 + 3) / 4)), dim3(256), 0, stream, (int)Nf0, (int)Nf1, (int)d, desc0, desc1, dNorm);
    for (int64_t a0 = 0; a0 < Nf0; a0 += H) {                    // bands ordered on the stream: each updates R in place
        const int h = (int)std::min<int64_t>(H, Nf0 - a0);
        const int64_t tiles = (int64_t)((h + STACK_TILE - 1) / STACK_TILE) * ((Nf1 + STACK_TILE - 1) / STACK_TILE);
        hipLaunchKernelGGL(k_stacked_band, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, (int)d, (int)a0, h, (int)Nf1, desc0, desc1,
                           (const double*)dNorm, (const double*)(dNorm + Nf0), Cb);
        hipLaunchKernelGGL(k_stacked_colmax, dim3((unsigned)((int64_t)S0 * nbx)), dim3(256), 0, stream, nbx, W0, (int)a0, h, (int)Nf1, a0 == 0 ? 1 : 0,
                           reinterpret_cast<const unsigned long long*>(mask0), (const double*)Cb, R);
    }
    hipLaunchKernelGGL(k_stacked_rowmax, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, (int)S0, (int)S1, W1, (int)Nf1,
                       reinterpret_cast<const unsigned long long*>(mask1), (const double*)R, sim);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_stacked_sim(roman_ctx_t* c, int32_t d, int32_t Nf0, const double* desc0, int32_t S0, const uint64_t* mask0,
                      int32_t Nf1, const double* desc1, int32_t S1, const uint64_t* mask1, double* sim)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    int rc = stacked_sim_check(c, d, Nf0, desc0, S0, mask0, Nf1, desc1, S1, mask1, sim);
    if (rc || S0 == 0 || S1 == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HostMirror m(c);
    const auto d0 = m.in(desc0, 8 * (size_t)Nf0 * (size_t)d), d1 = m.in(desc1, 8 * (size_t)Nf1 * (size_t)d);
    const auto m0 = m.in(mask0, 8 * (size_t)S0 * (((size_t)Nf0 + 63) / 64)), m1 = m.in(mask1, 8 * (size_t)S1 * (((size_t)Nf1 + 63) / 64));
    const auto dSim = m.out(sim, 8 * (size_t)S0 * (size_t)S1);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_stacked_sim_dev(c, d, Nf0, d0.dev(), S0, m0.dev(), Nf1, d1.dev(), S1, m1.dev(), dSim.dev());
    if (rc) return rc;
    return m.download();
}

// --- the stacked similarity of every block of a session in one launch sequence -----------------------------------
// One live block (submaps and frames on both sides) as the host sees it while it cuts the items.
struct SsLive { int32_t b; int64_t n0, Nf0, Nf1, r_off, a; };

// every view's frames inside the table of Nf frames, no negative mask offset
static int session_views_check(roman_ctx* c, int32_t Nf, int32_t R, const int32_t* frame_lo, const int32_t* frame_n, const int64_t* mask_off)
{
    for (int r = 0; r < R; ++r) {
        if (frame_lo[r] < 0 || frame_n[r] < 0 || (int64_t)frame_lo[r] + frame_n[r] > (int64_t)Nf)
            return fail(c, ROMAN_E_INVALID, "view %d: the frames [%d, %d + %d) leave the table of %d", r, frame_lo[r], frame_lo[r], frame_n[r], Nf);
        if (mask_off[r] < 0) return fail(c, ROMAN_E_INVALID, "view %d: mask_off=%lld is negative", r, (long long)mask_off[r]);
    }
    return ROMAN_OK;
}

// The tables are checked on their HOST copies (no read-back).  -> *total = pair_off[nb], the live blocks with their R offsets,
// *r_total: the doubles of all R together
static int session_stacked_check(roman_ctx* c, int32_t d, int32_t Nf, const void* desc, const void* mask, int32_t R, const int32_t* frame_lo,
                                 const int32_t* frame_n, const int64_t* mask_off, const int32_t* sub_off, int32_t nb, const int32_t* blocks,
                                 const int64_t* pair_off, const void* sim, int64_t* total, std::vector<SsLive>* live, int64_t* r_total)
{
    if (d < 1) return fail(c, ROMAN_E_INVALID, "d=%d: a frame descriptor has at least one component", d);
    if (Nf < 0 || R < 0 || nb < 0) return fail(c, ROMAN_E_INVALID, "Nf < 0, R < 0 or nb < 0");
    if (!sub_off || !pair_off || (nb > 0 && !blocks) || (R > 0 && (!frame_lo || !frame_n || !mask_off)))
        return fail(c, ROMAN_E_INVALID, "sub_off / blocks / pair_off / frame_lo / frame_n / mask_off is NULL");
    { int rc = session_views_check(c, Nf, R, frame_lo, frame_n, mask_off); if (rc) return rc; }
    int64_t tiles = 0; bool self = false;
    { int rc = session_tables_check(c, R, sub_off, nb, blocks, pair_off, nullptr, total, &tiles, &self); if (rc) return rc; }
    if (*total == 0) return ROMAN_OK;
    int64_t wgs = 0, tl = 0, ro = 0;
    for (int b = 0; b < nb; ++b) {
        const int32_t r0 = blocks[4 * b], r1 = blocks[4 * b + 1];
        const int64_t n0 = sub_off[r0 + 1] - sub_off[r0], n1 = sub_off[r1 + 1] - sub_off[r1], Nf0 = frame_n[r0], Nf1 = frame_n[r1];
        if (n0 == 0 || n1 == 0 || Nf0 == 0 || Nf1 == 0) continue;
        live->push_back(SsLive{b, n0, Nf0, Nf1, ro, 0});
        ro += n0 * Nf1;                                          // (n0 <= INT32_MAX / 16, Nf1 < 2^31, nb < 2^31: far inside int64)
        wgs += n0 * ((Nf1 + 255) / 256);
        tl += ((Nf0 + STACK_TILE - 1) / STACK_TILE) * ((Nf1 + STACK_TILE - 1) / STACK_TILE);
        if (wgs > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "the blocks' submaps x ceil(frames / 256) exceed the launch width of a round");
        if (tl > (int64_t)INT32_MAX) return fail(c, ROMAN_E_TOO_LARGE, "the blocks' frame-cosine matrices hold more than %d tiles", INT32_MAX);
    }
    *r_total = ro;
    if (!sim) return fail(c, ROMAN_E_INVALID, "sim is NULL");
    if (!live->empty() && (!desc || !mask)) return fail(c, ROMAN_E_INVALID, "desc / mask is NULL");
    return ROMAN_OK;
}

int roman_session_stacked_sim_dev(roman_ctx_t* c, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask,
                                  int32_t R, const int32_t* frame_lo, const int32_t* frame_lo_host, const int32_t* frame_n, const int32_t* frame_n_host,
                                  const int64_t* mask_off, const int64_t* mask_off_host, const int32_t* sub_off, const int32_t* sub_off_host,
                                  int32_t nb, const int32_t* blocks, const int32_t* blocks_host, const int64_t* pair_off, const int64_t* pair_off_host,
                                  double* sim)
{
    // (the arguments are judged first — on host memory only, a NULL context included, as roman_session_gate_dev does)
    if (!sub_off || !pair_off || (nb > 0 && !blocks) || (R > 0 && (!frame_lo || !frame_n || !mask_off))) return fail(c, ROMAN_E_INVALID, "a table is NULL on the device");
    int64_t total = 0, r_total = 0;
    std::vector<SsLive> live;
    int rc = session_stacked_check(c, d, Nf, desc, mask, R, frame_lo_host, frame_n_host, mask_off_host, sub_off_host, nb, blocks_host, pair_off_host, sim,
                                   &total, &live, &r_total);
    if (rc) return rc;
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (total == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;

    // ---- the items, round by round: at most one per block and round, a round's bands side by side within the budget (a forced band
    // height caps h; the first item of a round takes STACK_TILE rows at least, whatever they cost) ----
    struct Round { size_t it0, it1; int64_t tiles, wgs; };
    std::vector<SsItem> items;
    std::vector<Round> rounds;
    const int64_t budget = (int64_t)(64 << 20) / 8;
    int64_t bandMax = 0;
    for (size_t open = live.size(); open > 0;) {
        Round rd{items.size(), 0, 0, 0};
        int64_t used = 0;
        for (SsLive& L : live) {
            if (L.a >= L.Nf0) continue;
            int64_t h = ((budget - used) / L.Nf1) / STACK_TILE * STACK_TILE;
            if (c->stacked_band > 0) h = std::min<int64_t>(h, c->stacked_band);
            if (h < STACK_TILE) { if (used > 0) continue; h = STACK_TILE; }     // (no room left in this round: the block waits for the next)
            h = std::min(h, L.Nf0 - L.a);
            items.push_back(SsItem{used, rd.tiles, L.r_off, (int32_t)rd.wgs, L.b, (int32_t)L.a, (int32_t)h});
            used += h * L.Nf1;
            rd.tiles += ((h + STACK_TILE - 1) / STACK_TILE) * ((L.Nf1 + STACK_TILE - 1) / STACK_TILE);
            rd.wgs += L.n0 * ((L.Nf1 + 255) / 256);
            L.a += h;
            if (L.a >= L.Nf0) --open;
        }
        rd.it1 = items.size();
        bandMax = std::max(bandMax, used);
        rounds.push_back(rd);
    }

    // ---- scratch and staging first: a failure leaves nothing enqueued ----
    const size_t words = (size_t)nb + 5 * items.size();
    int64_t* staged = nullptr;
    HIPCHK(c, c->ssStage.stage(words, &staged));
    HIPCHK(c, c->ssItems.ensure(sizeof(int64_t) * words));
    HIPCHK(c, c->ssNorm.ensure(sizeof(double) * (size_t)std::max<int32_t>(Nf, 1)));
    HIPCHK(c, c->ssBand.ensure(sizeof(double) * (size_t)std::max<int64_t>(bandMax, 1)));
    HIPCHK(c, c->ssR.ensure(sizeof(double) * (size_t)std::max<int64_t>(r_total, 1)));
    std::fill(staged, staged + nb, (int64_t)0);
    for (const SsLive& L : live) staged[L.b] = L.r_off;
    if (!items.empty()) memcpy(staged + nb, items.data(), sizeof(SsItem) * items.size());
    HIPCHK(c, c->ssStage.upload(c->ssItems, words, stream));
    const int64_t* dRoff = c->ssItems.as<int64_t>();
    const SsItem* dItems = reinterpret_cast<const SsItem*>(dRoff + nb);
    double* const dNorm = c->ssNorm.as<double>();
    double* const band = c->ssBand.as<double>();
    double* const Rw = c->ssR.as<double>();
    const SsTab tab{(int)nb, sub_off, blocks, pair_off, frame_lo, frame_n, mask_off};
    const unsigned long long* m = reinterpret_cast<const unsigned long long*>(mask);
    if (!live.empty())                                           // once per frame of the session, whatever number of blocks and views read it
        hipLaunchKernelGGL(k_grid_norms, dim3((unsigned)(((int64_t)Nf + 3) / 4)), dim3(256), 0, stream, (int)Nf, 0, (int)d, desc, (const double*)nullptr, dNorm);
    for (const Round& rd : rounds) {                             // rounds ordered on the stream: each updates the blocks' R in place
        const int n = (int)(rd.it1 - rd.it0);
        hipLaunchKernelGGL(k_session_band, dim3((unsigned)((rd.tiles + 3) / 4)), dim3(256), 0, stream, (int)d, tab, dItems + rd.it0, n, rd.tiles, desc,
                           (const double*)dNorm, band);
        hipLaunchKernelGGL(k_session_colmax, dim3((unsigned)rd.wgs), dim3(256), 0, stream, tab, dItems + rd.it0, n, m, (const double*)band, Rw);
    }
    hipLaunchKernelGGL(k_session_rowmax, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, tab, dRoff, total, m, (const double*)Rw, sim);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_session_stacked_sim(roman_ctx_t* c, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask, int64_t mask_words,
                              int32_t R, const int32_t* frame_lo, const int32_t* frame_n, const int64_t* mask_off, const int32_t* sub_off,
                              int32_t nb, const int32_t* blocks, const int64_t* pair_off, double* sim)
{
    int64_t total = 0, r_total = 0;
    std::vector<SsLive> live;
    int rc = session_stacked_check(c, d, Nf, desc, mask, R, frame_lo, frame_n, mask_off, sub_off, nb, blocks, pair_off, sim, &total, &live, &r_total);
    if (rc) return rc;
    if (mask_words < 0) return fail(c, ROMAN_E_INVALID, "mask_words=%lld is negative", (long long)mask_words);
    for (int r = 0; r < R; ++r)                                  // the host twin copies `mask`: every view must lie inside the words it was given
        if (mask_off[r] + (int64_t)(sub_off[r + 1] - sub_off[r]) * (((int64_t)frame_n[r] + 63) / 64) > mask_words)
            return fail(c, ROMAN_E_INVALID, "view %d: its masks leave the %lld words of mask", r, (long long)mask_words);
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (total == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HostMirror m(c);
    const auto dDesc = m.in(desc, 8 * (size_t)Nf * (size_t)d);
    const auto dMask = m.in(mask, 8 * (size_t)mask_words);
    const auto dLo = m.in(frame_lo, 4 * (size_t)R), dN = m.in(frame_n, 4 * (size_t)R);
    const auto dMo = m.in(mask_off, 8 * (size_t)R);
    const auto dSub = m.in(sub_off, 4 * ((size_t)R + 1)), dBlk = m.in(blocks, 16 * (size_t)nb);
    const auto dPo = m.in(pair_off, 8 * ((size_t)nb + 1));
    const auto dSim = m.out(sim, 8 * (size_t)total);
    rc = m.upload();
    if (rc) return rc;
    rc = roman_session_stacked_sim_dev(c, d, Nf, dDesc.dev(), dMask.dev(), R, dLo.dev(), frame_lo, dN.dev(), frame_n, dMo.dev(), mask_off, dSub.dev(), sub_off,
                                       nb, dBlk.dev(), blocks, dPo.dev(), pair_off, dSim.dev());
    if (rc) return rc;
    return m.download();
}

// --- the stacked similarity of a list of pairs of a session -------------------------------------------------------
// On host memory, in front of everything else: the tables (session_tables_check), then what roman_session_stacked_sim_dev refuses
// about d, the views and the pointers it needs, then the list as roman_session_gate_list_dev judges it, then sim.
// -> *live_out: a block has submaps and frames on both sides (only then are desc and mask read, by any kernel)
static int session_stacked_list_check(roman_ctx* c, int32_t d, int32_t Nf, const void* desc, const void* mask, int32_t R, const int32_t* frame_lo,
                                      const int32_t* frame_n, const int64_t* mask_off, const int32_t* sub_off, int32_t nb, const int32_t* blocks,
                                      const int64_t* pair_off, int32_t L, const int32_t* list_host, const void* sim, bool* live_out)
{
    if (Nf < 0 || R < 0 || nb < 0) return fail(c, ROMAN_E_INVALID, "Nf < 0, R < 0 or nb < 0");
    if (!sub_off || !pair_off || (nb > 0 && !blocks) || (R > 0 && (!frame_lo || !frame_n || !mask_off)))
        return fail(c, ROMAN_E_INVALID, "sub_off / blocks / pair_off / frame_lo / frame_n / mask_off is NULL");
    int64_t total = 0, tiles = 0; bool self = false;
    { int rc = session_tables_check(c, R, sub_off, nb, blocks, pair_off, nullptr, &total, &tiles, &self); if (rc) return rc; }
    if (d < 1) return fail(c, ROMAN_E_INVALID, "d=%d: a frame descriptor has at least one component", d);
    { int rc = session_views_check(c, Nf, R, frame_lo, frame_n, mask_off); if (rc) return rc; }
    bool live = false;                                           // a block with submaps and frames on both sides: desc and mask are read
    for (int b = 0; b < nb && !live; ++b) {
        const int32_t r0 = blocks[4 * b], r1 = blocks[4 * b + 1];
        live = sub_off[r0 + 1] > sub_off[r0] && sub_off[r1 + 1] > sub_off[r1] && frame_n[r0] > 0 && frame_n[r1] > 0;
    }
    *live_out = live;
    if (live && (!desc || !mask)) return fail(c, ROMAN_E_INVALID, "desc / mask is NULL");
    if (L < 0) return fail(c, ROMAN_E_INVALID, "L=%d is negative", L);
    if (L == 0) return ROMAN_OK;
    { int rc = session_pair_list_check(c, sub_off, nb, blocks, L, list_host); if (rc) return rc; }
    if (!sim) return fail(c, ROMAN_E_INVALID, "sim is NULL with L=%d", L);
    return ROMAN_OK;
}

int roman_session_stacked_sim_list_dev(roman_ctx_t* c, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask,
                                       int32_t R, const int32_t* frame_lo, const int32_t* frame_lo_host, const int32_t* frame_n, const int32_t* frame_n_host,
                                       const int64_t* mask_off, const int64_t* mask_off_host, const int32_t* sub_off, const int32_t* sub_off_host,
                                       int32_t nb, const int32_t* blocks, const int32_t* blocks_host, const int64_t* pair_off, const int64_t* pair_off_host,
                                       int32_t L, const int32_t* list, const int32_t* list_host, double* sim)
{
    // (the arguments are judged first — on host memory only, a NULL context included — and the host copies in front of the device
    // pointers: the stated order of the refusals holds whatever the device pointers are)
    bool live = false;
    int rc = session_stacked_list_check(c, d, Nf, desc, mask, R, frame_lo_host, frame_n_host, mask_off_host, sub_off_host, nb, blocks_host, pair_off_host,
                                        L, list_host, sim, &live);
    if (rc) return rc;
    if (!sub_off || !pair_off || (nb > 0 && !blocks) || (R > 0 && (!frame_lo || !frame_n || !mask_off)) || (L > 0 && !list))
        return fail(c, ROMAN_E_INVALID, "a table or the list is NULL on the device");
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (L == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    HIPCHK(c, c->ssNorm.ensure(sizeof(double) * (size_t)std::max<int32_t>(Nf, 1)));     // scratch first: a failure leaves nothing enqueued
    double* const dNorm = c->ssNorm.as<double>();
    const SsTab tab{(int)nb, sub_off, blocks, pair_off, frame_lo, frame_n, mask_off};
    if (live)                                                    // once per frame of the session, over the frame table as it stands; without a
                                                                 // live block no pair reads a frame, and desc may be NULL
        hipLaunchKernelGGL(k_grid_norms, dim3((unsigned)(((int64_t)Nf + 3) / 4)), dim3(256), 0, stream, (int)Nf, 0, (int)d, desc, (const double*)nullptr, dNorm);
    hipLaunchKernelGGL(k_session_stacked_list, dim3((unsigned)(((int64_t)L + 3) / 4)), dim3(256), 0, stream, (int)d, tab, (int)L, list, desc, (const double*)dNorm,
                       reinterpret_cast<const unsigned long long*>(mask), sim);
    HIPCHK(c, hipGetLastError());
    return ROMAN_OK;
}

int roman_session_stacked_sim_list(roman_ctx_t* c, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask, int64_t mask_words,
                                   int32_t R, const int32_t* frame_lo, const int32_t* frame_n, const int64_t* mask_off, const int32_t* sub_off,
                                   int32_t nb, const int32_t* blocks, const int64_t* pair_off, int32_t L, const int32_t* list, double* sim)
{
    bool live = false;
    int rc = session_stacked_list_check(c, d, Nf, desc, mask, R, frame_lo, frame_n, mask_off, sub_off, nb, blocks, pair_off, L, list, sim, &live);
    if (rc) return rc;
    if (mask_words < 0) return fail(c, ROMAN_E_INVALID, "mask_words=%lld is negative", (long long)mask_words);
    for (int r = 0; r < R; ++r)                                  // the host twin copies `mask`: every view must lie inside the words it was given
        if (mask_off[r] + (int64_t)(sub_off[r + 1] - sub_off[r]) * (((int64_t)frame_n[r] + 63) / 64) > mask_words)
            return fail(c, ROMAN_E_INVALID, "view %d: its masks leave the %lld words of mask", r, (long long)mask_words);
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (L == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HostMirror m(c);
    // (without a live block desc and mask are not read and may be NULL: nothing of them goes up)
    const auto dDesc = m.in(desc, live ? 8 * (size_t)Nf * (size_t)d : 0);
    const auto dMask = m.in(mask, live ? 8 * (size_t)mask_words : 0);
    const auto dLo = m.in(frame_lo, 4 * (size_t)R), dN = m.in(frame_n, 4 * (size_t)R);
    const auto dMo = m.in(mask_off, 8 * (size_t)R);
    const auto dSub = m.in(sub_off, 4 * ((size_t)R + 1)), dBlk = m.in(blocks, 16 * (size_t)nb), dList = m.in(list, 12 * (size_t)L);
    const auto dPo = m.in(pair_off, 8 * ((size_t)nb + 1));
    const auto dSim = m.inout(sim, 8 * (size_t)pair_off[nb]);    // the caller's sim goes up first: the unlisted entries come back as they were
    rc = m.upload();
    if (rc) return rc;
    rc = roman_session_stacked_sim_list_dev(c, d, Nf, dDesc.dev(), dMask.dev(), R, dLo.dev(), frame_lo, dN.dev(), frame_n, dMo.dev(), mask_off, dSub.dev(), sub_off,
                                            nb, dBlk.dev(), blocks, dPo.dev(), pair_off, L, dList.dev(), list, dSim.dev());
    if (rc) return rc;
    return m.download();
}

// --- the deal of a batch over ranks (pure host function; roman_amd.align.distributed.deal_by_cost states the same) ------------
int roman_deal_problems(int32_t B, const int32_t* n1, const int32_t* n2, const int64_t* assoc_off,
                        int32_t world, int32_t rank, int32_t* idx_out, int32_t* n_out)
{
    if (B < 0 || world < 1 || rank < 0 || rank >= world || !n_out || (B > 0 && (!n1 || !n2 || !idx_out)))
        return fail(nullptr, ROMAN_E_INVALID, "bad arguments");
    std::vector<int64_t> work((size_t)B);
    for (int b = 0; b < B; ++b) {
        int64_t a = assoc_off ? assoc_off[b + 1] - assoc_off[b] : 0;
        if (a <= 0) a = (int64_t)n1[b] * n2[b];                 // no list, or an empty one: all-to-all
        work[(size_t)b] = a * a;
    }
    std::vector<int32_t> order((size_t)B);
    for (int b = 0; b < B; ++b) order[(size_t)b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return work[(size_t)x] > work[(size_t)y]; });
    std::vector<int64_t> load((size_t)world, 0), count((size_t)world, 0);
    std::vector<int32_t> mine;
    for (int32_t b : order) {
        int r = 0;
        for (int t = 1; t < world; ++t)
            if (load[(size_t)t] < load[(size_t)r] || (load[(size_t)t] == load[(size_t)r] && count[(size_t)t] < count[(size_t)r])) r = t;
        load[(size_t)r] += std::max<int64_t>(work[(size_t)b], 1); count[(size_t)r] += 1;
        if (r == rank) mine.push_back(b);
    }
    std::sort(mine.begin(), mine.end());
    for (size_t t = 0; t < mine.size(); ++t) idx_out[t] = mine[t];
    *n_out = (int32_t)mine.size();
    return ROMAN_OK;
}

// --- stepwise surface for the clipperpy-compatible shim -----------------------------------------------
int roman_create_all_to_all(int32_t n1, int32_t n2, int32_t* out)
{
    if (n1 < 0 || n2 < 0 || (!out && (int64_t)n1 * n2 > 0)) return fail(nullptr, ROMAN_E_INVALID, "bad arguments");
    for (int32_t i = 0; i < n1; ++i) for (int32_t j = 0; j < n2; ++j) { out[2 * ((int64_t)i * n2 + j)] = i; out[2 * ((int64_t)i * n2 + j) + 1] = j; }
    return ROMAN_OK;
}

int roman_score(roman_ctx_t* c, const roman_params_t* params, const double* D1, int32_t n1,
                const double* D2, int32_t n2, int32_t F, const int32_t* assoc, int32_t n_assoc)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (n1 < 0 || n2 < 0 || F < 0 || (assoc && n_assoc < 0)) return fail(c, ROMAN_E_INVALID, "negative size");
    if ((n1 > 0 && !D1) || (n2 > 0 && !D2)) return fail(c, ROMAN_E_INVALID, "NULL feature matrix");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    roman_ctx::Last& Lst = c->last;
    Lst.scored = false; Lst.solved = false; Lst.dense = false; Lst.hascz = false;
    DevParams D0;
    int rc = make_dev_params(c, params, F, &D0);
    if (rc) return rc;
    const int64_t nobj = (int64_t)n1 + n2;
    HIPCHK(c, WS.hFeats.ensure(sizeof(double) * (size_t)std::max<int64_t>(nobj * F, 1)));
    if ((int64_t)n1 * F > 0) HIPCHK(c, hipMemcpyAsync(WS.hFeats.p, D1, sizeof(double) * (size_t)n1 * F, hipMemcpyHostToDevice, WS.stream));
    if ((int64_t)n2 * F > 0) HIPCHK(c, hipMemcpyAsync(WS.hFeats.as<double>() + (size_t)n1 * F, D2, sizeof(double) * (size_t)n2 * F, hipMemcpyHostToDevice, WS.stream));
    const int32_t* dA = nullptr;
    if (assoc && n_assoc == 0) assoc = nullptr;        // clipperpy: an empty A is replaced by the all-to-all list
    int64_t aoff[2] = {0, n_assoc};
    Lst.assoc.clear();
    if (assoc) {
        for (int32_t k = 0; k < n_assoc; ++k)
            if (assoc[2 * k] < 0 || assoc[2 * k] >= n1 || assoc[2 * k + 1] < 0 || assoc[2 * k + 1] >= n2)
                return fail(c, ROMAN_E_INVALID, "association %d = (%d,%d) out of range", k, assoc[2 * k], assoc[2 * k + 1]);
        Lst.assoc.assign(assoc, assoc + 2 * (size_t)n_assoc);
        HIPCHK(c, WS.hAssoc.ensure(sizeof(int32_t) * 2 * (size_t)std::max(n_assoc, 1)));
        if (n_assoc > 0) HIPCHK(c, hipMemcpyAsync(WS.hAssoc.p, assoc, sizeof(int32_t) * 2 * (size_t)n_assoc, hipMemcpyHostToDevice, WS.stream));
        dA = WS.hAssoc.as<int32_t>();
    }
    const int64_t o1 = 0, o2 = n1;
    const BatchIn in{1, WS.hFeats.as<double>(), &o1, &n1, &o2, &n2, F, dA, aoff};
    std::vector<ProbDesc> hd;
    ProbState ps{};
    for (int attempt = 0; ; ++attempt) {
        rc = enqueue_score(c, D0, params, in, hd, &Lst.D);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(&ps, WS.state.p, sizeof(ProbState), hipMemcpyDeviceToHost, WS.stream));
        HIPCHK(c, hipStreamSynchronize(WS.stream));
        if (!batch_overflowed(c)) break;
        if (attempt + 1 >= MAX_ATTEMPTS) return fail(c, ROMAN_E_NOMEM, "the sparse workspace still does not fit after %d attempts", attempt + 1);
    }
    Lst.pd = hd[0]; Lst.nA = hd[0].nA; Lst.L = ps.L; Lst.kind = ps.kind; Lst.nnzCap = ps.nnzCap; Lst.scored = true;
    return ROMAN_OK;
}

int roman_set_matrix_data(roman_ctx_t* c, const roman_params_t* params, const double* M, const double* Cm, int32_t n)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && (!M || !Cm))) return fail(c, ROMAN_E_INVALID, "bad matrix arguments");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    roman_ctx::Last& Lst = c->last;
    Lst.scored = false; Lst.solved = false; Lst.dense = true; Lst.assoc.clear();
    roman_params_t p = *params; p.invariant = ROMAN_INV_EUCLIDEAN;          // implicit identity diagonal
    int rc = make_dev_params(c, &p, p.point_dim, &Lst.D);
    if (rc) return rc;
    // The weights decide the solver.  The stream solver adds FIXED-POINT terms rint(v x 2^s) (kernels.hip.h, "Exact
    // accumulation"): a term stays below 2^50 and a row's sum below 2^62 only for 0 <= v <= 1 (what every scored matrix
    // holds by construction), and its accumulators are decoded as unsigned.  A caller's dense M may hold anything: the
    // strict upper triangle is scanned on the device first, and a matrix with a weight outside [0, 1] (or not finite) takes
    // the plain-double solvers of the fallback layout instead.
    const size_t n1_ = (size_t)std::max(n, 1);
    HIPCHK(c, WS.hAux1.ensure(sizeof(double) * n1_ * n1_)); HIPCHK(c, WS.hAux2.ensure(sizeof(double) * n1_ * n1_)); HIPCHK(c, WS.hAux3.ensure(sizeof(int) * 4));
    HIPCHK(c, hipMemsetAsync(WS.hAux3.p, 0, sizeof(int) * 4, WS.stream));
    int rangeFlag = 0;
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(WS.hAux1.p, M, sizeof(double) * n1_ * n1_, hipMemcpyHostToDevice, WS.stream));
        HIPCHK(c, hipMemcpyAsync(WS.hAux2.p, Cm, sizeof(double) * n1_ * n1_, hipMemcpyHostToDevice, WS.stream));
        hipLaunchKernelGGL(k_dense_range, dim3((unsigned)std::min(c->num_cu * 8, (n + 3) / 4)), dim3(256), 0, WS.stream, n, WS.hAux1.as<double>(), WS.hAux3.as<int>());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&rangeFlag, WS.hAux3.as<int>() + 1, sizeof(int), hipMemcpyDeviceToHost, WS.stream));
        HIPCHK(c, hipStreamSynchronize(WS.stream));
    }
    const bool iter = Lst.D.p.maxiniters >= 1 && Lst.D.p.maxlsiters >= 1;
    const bool up = n <= STREAM_MAXL && iter && rangeFlag == 0;
    // few large problems: the whole-device solver; a problem the range check keeps off the stream solver is small enough for
    // one workgroup (k_solve: u and u' in LDS)
    Lst.D.wide = (!up && n > STREAM_MAXL && c->coop_ok && iter && n <= (int64_t)WIDE_KW * c->num_cu * WIDE_NW * 64) ? 1 : 0;
    Lst.D.idx16 = 0;                                           // dense problems may carry C flags: 32-bit labels
    Lst.D.stream_maxL = up ? std::max(64, (n + 63) & ~63) : 64;
    // The conversion runs on the device (kernels.hip.h, "Dense problems"): upload M and C, candidate bit matrix, then the
    // scored path's own layout kernels.  Two small read-backs size the matrix pools (the slot total is known only after the
    // sort) and fetch the C-flag / capacity status.
    const int W = (n + 63) / 64;
    const int RPB = 128;
    const size_t maskWords = std::max<size_t>((size_t)n * (size_t)W, 1);
    const long long capList = up ? (long long)n * (n - 1) / 2 + 4LL * n + 4 : 4;
    HIPCHK(c, WS.probs.ensure(sizeof(ProbDesc))); HIPCHK(c, WS.state.ensure(sizeof(ProbState))); HIPCHK(c, WS.totals.ensure(sizeof(BatchTotals)));
    HIPCHK(c, WS.queue.ensure(sizeof(int) * 16));
    {
        DevBuf* i32s[] = {&WS.lp, &WS.plp, &WS.rowCnt, &WS.rowPos, &WS.perm, &WS.sliceWidth, &WS.sliceBase, &WS.listOff};
        for (DevBuf* b_ : i32s) HIPCHK(c, b_->ensure(sizeof(int32_t) * n1_));
        DevBuf* f64s[] = {&WS.ls, &WS.ld, &WS.pld};
        for (DevBuf* b_ : f64s) HIPCHK(c, b_->ensure(sizeof(double) * n1_));
    }
    HIPCHK(c, WS.maskPool.ensure(sizeof(unsigned long long) * maskWords)); HIPCHK(c, WS.prefPool.ensure(sizeof(uint32_t) * maskWords));
    HIPCHK(c, WS.listPool.ensure(sizeof(uint16_t) * (size_t)capList));
    HIPCHK(c, WS.items.ensure(sizeof(ItemDesc) * ((size_t)n / RPB + 2)));
    WS.capMaskWords = std::max<long long>(WS.capMaskWords, (long long)maskWords); WS.capList = std::max<long long>(WS.capList, capList);
    ProbDesc pd{}; pd.off1 = 0; pd.off2 = 0; pd.assocOff = -1; pd.liveOff = 0; pd.n1 = n; pd.n2 = 1; pd.nA = n;
    ProbState ps{}; ps.L = n; ps.kind = up ? 0 : 1;
    HIPCHK(c, hipMemcpyAsync(WS.probs.p, &pd, sizeof(pd), hipMemcpyHostToDevice, WS.stream));
    HIPCHK(c, hipMemcpyAsync(WS.state.p, &ps, sizeof(ps), hipMemcpyHostToDevice, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));                  // (pd, ps live on this frame)
    const ProbDesc* dP = WS.probs.as<ProbDesc>(); ProbState* dS = WS.state.as<ProbState>(); BatchTotals* dT = WS.totals.as<BatchTotals>();
    const double* dM = WS.hAux1.as<double>(); const double* dC = WS.hAux2.as<double>();
    if (n > 0) {
        std::vector<int32_t> ident(n1_); std::vector<double> ones(n1_, 1.0);
        for (int k = 0; k < n; ++k) ident[(size_t)k] = k;
        HIPCHK(c, hipMemcpy(WS.lp.p, ident.data(), sizeof(int32_t) * n1_, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(WS.plp.p, ident.data(), sizeof(int32_t) * n1_, hipMemcpyHostToDevice));      // (stream layout: k_upper overwrites it with the permutation)
        HIPCHK(c, hipMemcpy(WS.ls.p, ones.data(), sizeof(double) * n1_, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(WS.ld.p, ones.data(), sizeof(double) * n1_, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(WS.pld.p, ones.data(), sizeof(double) * n1_, hipMemcpyHostToDevice));
    }
    const LivePools LP{WS.lp.as<int32_t>(), nullptr, nullptr, WS.ls.as<double>(), WS.ld.as<double>(), nullptr, nullptr};
    const LivePools PP{WS.plp.as<int32_t>(), nullptr, nullptr, nullptr, WS.pld.as<double>(), nullptr, nullptr};
    hipLaunchKernelGGL(k_rowbase, dim3(1), dim3(256), 0, WS.stream, 1, RPB, (long long)maskWords, dS, dT, 0, (const int32_t*)nullptr);
    hipLaunchKernelGGL(k_items, dim3(1), dim3(256), 0, WS.stream, RPB, dS, WS.items.as<ItemDesc>());
    if (n > 0) {
        hipLaunchKernelGGL(k_dense_mask, dim3((unsigned)std::min(c->num_cu * 8, (n + 3) / 4)), dim3(256), 0, WS.stream, n, dM, dC,
                           WS.maskPool.as<unsigned long long>(), WS.hAux3.as<int>());
        hipLaunchKernelGGL(k_rowprefix, dim3(c->num_cu * 2), dim3(1024), 0, WS.stream, dP, dS, dT, WS.items.as<ItemDesc>(),
                           WS.maskPool.as<unsigned long long>(), WS.prefPool.as<uint32_t>(), WS.rowCnt.as<uint32_t>(), RPB, 0);
        hipLaunchKernelGGL(k_rowsort, dim3(1), dim3(1024), 0, WS.stream, dP, dS, dT, WS.rowCnt.as<uint32_t>(), WS.rowPos.as<uint32_t>(), WS.perm.as<uint32_t>(),
                           WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.listOff.as<uint32_t>(), capList, 0, read_switches().sort_eq_max);
        if (up) {
            hipLaunchKernelGGL(k_upper, dim3(c->num_cu * 2), dim3(1024), 0, WS.stream, dP, dS, dT, WS.items.as<ItemDesc>(),
                               WS.maskPool.as<unsigned long long>(), WS.listPool.as<uint16_t>(), WS.listOff.as<uint32_t>(),
                               WS.rowCnt.as<uint32_t>(), WS.perm.as<uint32_t>(), WS.rowPos.as<uint32_t>(), LP, PP, RPB);
            hipLaunchKernelGGL(k_slicegeom, dim3(1), dim3(64), 0, WS.stream, dP, dS, WS.rowCnt.as<uint32_t>(), WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>());
        }
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&ps, WS.state.p, sizeof(ps), hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    if (ps.kind == 2) return fail(c, ROMAN_E_NOMEM, "internal: dense problem does not fit its own workspace");
    const uint64_t total = ps.nnzCap;
    if (total > 4000000000ull) return fail(c, ROMAN_E_TOO_LARGE, "dense matrix has too many non-zeros");
    const size_t nnz1 = (size_t)std::max<uint64_t>(total, 1);
    HIPCHK(c, WS.vals.ensure(sizeof(double) * nnz1)); HIPCHK(c, WS.cols16.ensure(sizeof(uint16_t) * nnz1)); HIPCHK(c, WS.cols32.ensure(sizeof(uint32_t) * nnz1));
    WS.capNnz = std::max<long long>(WS.capNnz, (long long)nnz1);
    hipLaunchKernelGGL(k_probscan, dim3(1), dim3(256), 0, WS.stream, 1, 1, (long long)nnz1, dS, dT);
    if (total > 0) {
        const unsigned grid = (unsigned)std::min<uint64_t>((total + 255) / 256, (uint64_t)c->num_cu * 16);
        auto kf = up ? k_dense_fill<0> : k_dense_fill<1>;
        hipLaunchKernelGGL(kf, dim3(grid), dim3(256), 0, WS.stream, n, dM, dC, dS, WS.rowCnt.as<uint32_t>(), WS.rowPos.as<uint32_t>(), WS.perm.as<uint32_t>(),
                           WS.sliceWidth.as<uint32_t>(), WS.sliceBase.as<uint32_t>(), WS.listPool.as<uint16_t>(), WS.listOff.as<uint32_t>(),
                           WS.maskPool.as<unsigned long long>(), WS.prefPool.as<uint32_t>(), WS.cols16.as<uint16_t>(), WS.cols32.as<uint32_t>(), WS.vals.as<double>());
    }
    HIPCHK(c, hipGetLastError());
    int flags[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&ps, WS.state.p, sizeof(ps), hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipMemcpyAsync(flags, WS.hAux3.p, sizeof(flags), hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    if (ps.kind == 2) return fail(c, ROMAN_E_NOMEM, "internal: dense problem does not fit its own workspace");
    Lst.hascz = flags[0] != 0;
    Lst.pd = pd; Lst.nA = n; Lst.L = n; Lst.kind = ps.kind; Lst.nnzCap = (int64_t)total;
    Lst.scored = true;
    return ROMAN_OK;
}

int roman_solve(roman_ctx_t* c, const double* u0)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (!c->last.scored) return fail(c, ROMAN_E_INVALID, "roman_solve: no matrices (call roman_score or roman_set_matrix_data first)");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    return solve_last(c, u0);
}

int roman_num_associations(const roman_ctx_t* c, int32_t* n)
{
    if (!c || !n) return fail(nullptr, ROMAN_E_INVALID, "NULL argument");
    if (!c->last.scored) return fail(const_cast<roman_ctx*>(c), ROMAN_E_INVALID, "nothing scored yet");
    *n = c->last.nA; return ROMAN_OK;
}
int roman_num_selected(const roman_ctx_t* c, int32_t* n)
{
    if (!c || !n) return fail(nullptr, ROMAN_E_INVALID, "NULL argument");
    if (!c->last.solved) return fail(const_cast<roman_ctx*>(c), ROMAN_E_INVALID, "nothing solved yet");
    *n = c->last.nsel; return ROMAN_OK;
}
int roman_get_selected_associations(const roman_ctx_t* c, int32_t* out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const roman_ctx::Last& L = c->last;
    if (!L.solved) return fail(const_cast<roman_ctx*>(c), ROMAN_E_INVALID, "nothing solved yet");
    for (int32_t t = 0; t < L.nsel; ++t) {
        const int32_t p = L.nodes[(size_t)t];
        if (!L.assoc.empty()) { out[2 * t] = L.assoc[2 * (size_t)p]; out[2 * t + 1] = L.assoc[2 * (size_t)p + 1]; }
        else if (L.dense) { out[2 * t] = p; out[2 * t + 1] = p; }
        else { out[2 * t] = p / L.pd.n2; out[2 * t + 1] = p % L.pd.n2; }
    }
    return ROMAN_OK;
}
int roman_get_solution(const roman_ctx_t* c, int32_t* nodes, double* u, double* score, roman_stats_t* stats)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const roman_ctx::Last& L = c->last;
    if (!L.solved) return fail(const_cast<roman_ctx*>(c), ROMAN_E_INVALID, "nothing solved yet");
    if (nodes) for (int32_t t = 0; t < L.nsel; ++t) nodes[t] = L.nodes[(size_t)t];
    if (u) for (int32_t p = 0; p < L.nA; ++p) u[p] = L.u[(size_t)p];
    if (score) *score = L.stats.score;
    if (stats) *stats = L.stats;
    return ROMAN_OK;
}

int roman_get_upper_csr(const roman_ctx_t* c, int64_t* nnz, int64_t* rowptr, int32_t* cols_out, double* vals_out, double* diag)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const roman_ctx::Last& Lst = c->last;
    if (!Lst.scored) return fail(const_cast<roman_ctx*>(c), ROMAN_E_INVALID, "nothing scored yet");
    std::vector<uint32_t> rs, rl, cols; std::vector<double> vals, ls; std::vector<int32_t> lp;
    int rc = fetch_last_csr(c, rs, rl, cols, vals, lp, ls);
    if (rc) return rc;
    const int L = Lst.L, nA = Lst.nA;
    int64_t cnt = 0;
    std::vector<int64_t> rp((size_t)nA + 1, 0);
    for (int k = 0; k < L; ++k) {
        int64_t rc_ = 0;
        for (uint32_t e = 0; e < rl[(size_t)k]; ++e) { const uint32_t q = cols[(size_t)rs[(size_t)k] + e] & 0x7fffffffu; if ((int)q > k) ++rc_; }
        rp[(size_t)lp[(size_t)k] + 1] = rc_; cnt += rc_;
    }
    for (int p = 0; p < nA; ++p) rp[(size_t)p + 1] += rp[(size_t)p];
    if (nnz) *nnz = cnt;
    if (rowptr) for (int p = 0; p <= nA; ++p) rowptr[p] = rp[(size_t)p];
    if (cols_out || vals_out) {
        for (int k = 0; k < L; ++k) {
            int64_t w = rp[(size_t)lp[(size_t)k]];
            for (uint32_t e = 0; e < rl[(size_t)k]; ++e) {
                const uint32_t q = cols[(size_t)rs[(size_t)k] + e] & 0x7fffffffu;
                if ((int)q > k) { if (cols_out) cols_out[w] = lp[(size_t)q]; if (vals_out) vals_out[w] = vals[(size_t)rs[(size_t)k] + e]; ++w; }
            }
        }
    }
    if (diag) {
        const bool single = Lst.D.single && !Lst.dense;
        for (int p = 0; p < nA; ++p) diag[p] = single ? 0.0 : 1.0;
        if (single) for (int k = 0; k < L; ++k) diag[(size_t)lp[(size_t)k]] = ls[(size_t)k];
    }
    return ROMAN_OK;
}

int roman_get_dense_matrices(const roman_ctx_t* c, double* M, double* Cm)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    const roman_ctx::Last& Lst = c->last;
    if (!Lst.scored) return fail(const_cast<roman_ctx*>(c), ROMAN_E_INVALID, "nothing scored yet");
    std::vector<uint32_t> rs, rl, cols; std::vector<double> vals, ls; std::vector<int32_t> lp;
    int rc = fetch_last_csr(c, rs, rl, cols, vals, lp, ls);
    if (rc) return rc;
    const int L = Lst.L; const int64_t nA = Lst.nA;
    if (M) memset(M, 0, sizeof(double) * (size_t)(nA * nA));
    if (Cm) memset(Cm, 0, sizeof(double) * (size_t)(nA * nA));
    const bool single = Lst.D.single && !Lst.dense;
    for (int64_t p = 0; p < nA; ++p) { if (M) M[p * nA + p] = single ? 0.0 : 1.0; if (Cm) Cm[p * nA + p] = 1.0; }
    for (int k = 0; k < L; ++k) {
        const int64_t p = lp[(size_t)k];
        if (single && M) M[p * nA + p] = ls[(size_t)k];
        for (uint32_t e = 0; e < rl[(size_t)k]; ++e) {
            const uint32_t cq = cols[(size_t)rs[(size_t)k] + e];
            const int64_t q = lp[(size_t)(cq & 0x7fffffffu)];
            if (M) M[p * nA + q] = vals[(size_t)rs[(size_t)k] + e];
            if (Cm) Cm[p * nA + q] = (cq & 0x80000000u) ? 0.0 : 1.0;
        }
    }
    return ROMAN_OK;
}

// --- pose from given correspondences -----------------------------------------------------------------
int roman_pose_batch(roman_ctx_t* c, int32_t dim, int32_t B, const double* pts1, const double* pts2,
                     const int64_t* corr_off, double* T_out, int32_t* status_out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (dim != 2 && dim != 3) return fail(c, ROMAN_E_INVALID, "dim must be 2 or 3");
    if (B < 0 || !corr_off || !T_out || !status_out) return fail(c, ROMAN_E_INVALID, "bad arguments");
    if (B == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    const int64_t K = corr_off[B];
    if (K < 0 || (K > 0 && (!pts1 || !pts2))) return fail(c, ROMAN_E_INVALID, "bad correspondence arrays");
    HIPCHK(c, WS.hAux1.ensure(sizeof(double) * (size_t)std::max<int64_t>(K * dim, 1)));
    HIPCHK(c, WS.hAux2.ensure(sizeof(double) * (size_t)std::max<int64_t>(K * dim, 1)));
    HIPCHK(c, WS.hAux3.ensure(sizeof(int64_t) * ((size_t)B + 1)));
    HIPCHK(c, WS.oT.ensure(sizeof(double) * 16 * (size_t)B)); HIPCHK(c, WS.oStatus.ensure(sizeof(int32_t) * (size_t)B));
    if (K > 0) {
        HIPCHK(c, hipMemcpyAsync(WS.hAux1.p, pts1, sizeof(double) * (size_t)(K * dim), hipMemcpyHostToDevice, WS.stream));
        HIPCHK(c, hipMemcpyAsync(WS.hAux2.p, pts2, sizeof(double) * (size_t)(K * dim), hipMemcpyHostToDevice, WS.stream));
    }
    HIPCHK(c, hipMemcpyAsync(WS.hAux3.p, corr_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyHostToDevice, WS.stream));
    hipLaunchKernelGGL(k_pose, dim3(B), dim3(64), 0, WS.stream, dim, WS.hAux1.as<double>(), WS.hAux2.as<double>(), WS.hAux3.as<int64_t>(),
                       WS.oT.as<double>(), WS.oStatus.as<int32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(T_out, WS.oT.p, sizeof(double) * 16 * (size_t)B, hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipMemcpyAsync(status_out, WS.oStatus.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    return ROMAN_OK;
}

// --- diagnostics -------------------------------------------------------------------------------------------
int roman_debug_math(roman_ctx_t* c, int kind, const double* in1, const double* in2, int64_t n, double* out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && (!in1 || !out))) return fail(c, ROMAN_E_INVALID, "bad arguments");
    if (n == 0) return ROMAN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    HIPCHK(c, WS.hAux1.ensure(sizeof(double) * (size_t)n)); HIPCHK(c, WS.hAux2.ensure(sizeof(double) * (size_t)n)); HIPCHK(c, WS.hAux3.ensure(sizeof(double) * (size_t)n));
    HIPCHK(c, hipMemcpyAsync(WS.hAux1.p, in1, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, WS.stream));
    if (in2) HIPCHK(c, hipMemcpyAsync(WS.hAux2.p, in2, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, WS.stream));
    hipLaunchKernelGGL(k_debug_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, WS.stream, kind, WS.hAux1.as<double>(),
                       in2 ? WS.hAux2.as<double>() : (const double*)nullptr, n, WS.hAux3.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, WS.hAux3.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    return ROMAN_OK;
}

int roman_debug_cosine(roman_ctx_t* c, const roman_params_t* params, const double* D1, int32_t n1,
                       const double* D2, int32_t n2, int32_t F, double* out)
{
    if (!c) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    if (n1 <= 0 || n2 <= 0 || !D1 || !D2 || !out) return fail(c, ROMAN_E_INVALID, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc0 = use_ws0(c); if (rc0) return rc0; }
    DevParams D;
    int rc = make_dev_params(c, params, F, &D);
    if (rc) return rc;
    if (D.p.cos_feature_dim <= 0) return fail(c, ROMAN_E_INVALID, "cos_feature_dim is 0");
    HIPCHK(c, WS.hFeats.ensure(sizeof(double) * (size_t)(n1 + n2) * F));
    HIPCHK(c, hipMemcpyAsync(WS.hFeats.p, D1, sizeof(double) * (size_t)n1 * F, hipMemcpyHostToDevice, WS.stream));
    HIPCHK(c, hipMemcpyAsync(WS.hFeats.as<double>() + (size_t)n1 * F, D2, sizeof(double) * (size_t)n2 * F, hipMemcpyHostToDevice, WS.stream));
    ProbDesc pd{}; pd.off1 = 0; pd.off2 = n1; pd.assocOff = -1; pd.n1 = n1; pd.n2 = n2; pd.nA = n1 * n2;
    HIPCHK(c, WS.probs.ensure(sizeof(ProbDesc)));
    HIPCHK(c, WS.cosPool.ensure(sizeof(double) * (size_t)n1 * n2));
    HIPCHK(c, hipMemcpyAsync(WS.probs.p, &pd, sizeof(pd), hipMemcpyHostToDevice, WS.stream));
    // sw.cos_sel_matrix approx / gated (tests): k_cos_sel's screen matrix / k_cos_sel's matrix (exact where cos >= cosine_min - 2^-6, the screen elsewhere)
    const Switches sw = read_switches();
    if (sw.cos_sel_matrix && n1 <= CSEL_MAXN && n2 <= CSEL_MAXN) {
        HIPCHK(c, WS.cosDense.ensure(sizeof(int32_t)));
        HIPCHK(c, launch_cos_sel(c, WS.stream, D, 1, n1, n2, WS.probs.as<ProbDesc>(), WS.hFeats.as<double>(), WS.cosPool.as<double>(), WS.cosDense.as<int32_t>(), sw.cos_sel_matrix == COS_SEL_APPROX));
    } else
    HIPCHK(c, launch_cos(c, sw, WS.stream, D, 1, n1, n2, WS.probs.as<ProbDesc>(), WS.hFeats.as<double>(), WS.cosPool.as<double>()));
    HIPCHK(c, hipMemcpyAsync(out, WS.cosPool.p, sizeof(double) * (size_t)n1 * n2, hipMemcpyDeviceToHost, WS.stream));
    HIPCHK(c, hipStreamSynchronize(WS.stream));
    c->last.scored = false; c->last.solved = false;
    return ROMAN_OK;
}

int roman_debug_live(const roman_ctx_t* cc, int32_t* n_live, int32_t* idx, double* score)
{
    if (!cc) return fail(nullptr, ROMAN_E_INVALID, "ctx is NULL");
    roman_ctx* c = const_cast<roman_ctx*>(cc);
    if (!c->last.scored) return fail(c, ROMAN_E_INVALID, "nothing scored yet");
    const int L = c->last.L;
    if (n_live) *n_live = L;
    HIPCHK(c, hipSetDevice(c->device));
    if (idx && L > 0) HIPCHK(c, hipMemcpy(idx, WS.lp.p, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost));
    if (score && L > 0) HIPCHK(c, hipMemcpy(score, WS.ls.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost));
    return ROMAN_OK;
}

}  // extern "C"
