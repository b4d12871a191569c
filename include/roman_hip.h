/*
 * roman_hip.h — C ABI of libroman_hip.so, the MI355X (gfx950) replacement for the
 * `clipperpy` native module that mit-acl/roman's `roman.align` hot path binds.
 *
 * Every entry point names the reference interface it replaces ([REF file:line] is relative
 * to the reference checkout).  Plain pointers and sizes only: no torch / numpy / C++ types
 * cross this boundary.  All functions return 0 on success or a negative ROMAN_E_* code; they
 * never throw.  The library fails (ROMAN_E_NO_DEVICE) when no HIP device is present — there
 * is no CPU fallback behind this ABI.
 *
 * Data conventions (same as the reference's calls into clipperpy):
 *   - A "feature matrix" is what [REF roman/align/roman_registration.py:91-95] hands to
 *     `score_pairwise_and_single_consistency` as `map_cl.T`: F x n float64, one COLUMN per
 *     object, column-major == object-major: object o's F features are the F contiguous
 *     doubles at feats[o*F .. o*F+F).  Row layout inside a column is
 *     [x y (z)] ++ ratio features (ratio_feature_dim) ++ cosine features (cos_feature_dim)
 *     [REF roman/align/roman_registration.py:98-108].
 *   - An association list is (A,2) int32 row-major; column 0 indexes map 1, column 1 map 2
 *     [REF roman/align/object_registration.py:110-111].  A NULL list means all-to-all in
 *     the order of clipperpy.utils.create_all_to_all: row i*n2+j = (i,j)
 *     [REF roman/align/object_registration.py:41].
 *   - A pose is a row-major (dim+1)x(dim+1) float64 matrix mapping map 2 into map 1
 *     [REF roman/align/object_registration.py:88-129]; always stored in 16 doubles.
 */
#ifndef ROMAN_HIP_H
#define ROMAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exported from libroman_hip.so (the library is built with -fvisibility=hidden) */
#if defined(__GNUC__)
#define ROMAN_API __attribute__((visibility("default")))
#else
#define ROMAN_API
#endif

#define ROMAN_MAX_RATIO_FEATURES 8

/* error codes */
#define ROMAN_OK                0
#define ROMAN_E_INVALID        -1   /* bad argument (NULL pointer, dim not 2/3, ...)            */
#define ROMAN_E_NO_DEVICE      -2   /* no HIP device / wrong architecture                        */
#define ROMAN_E_HIP            -3   /* a HIP runtime call failed (see roman_last_error)          */
#define ROMAN_E_NOMEM          -4   /* device or host allocation failed                          */
#define ROMAN_E_UNSUPPORTED    -5   /* parameter combination the reference does not define       */
#define ROMAN_E_TOO_LARGE      -6   /* problem exceeds the index width of this build             */
#define ROMAN_E_INTERNAL       -7   /* a problem came back with ROMAN_ST_INTERNAL (host-pointer / stepwise entry points; the
                                       outputs have been copied: status_out says which problems have no result)           */

/* per-problem status written to status_out[] (bit flags) */
#define ROMAN_ST_OK                  0
#define ROMAN_ST_EMPTY_MAP           1  /* n1==0 or n2==0: register() returns (1,0) array [REF object_registration.py:23-24] */
#define ROMAN_ST_INSUFFICIENT        2  /* fewer than `dim` associations: T_align raises InsufficientAssociationsException [REF object_registration.py:107-108] */
#define ROMAN_ST_MAXITER             4  /* solver stopped on maxoliters                          */
#define ROMAN_ST_ASSOC_TRUNCATED     8  /* more selected associations than kmax (output clipped) */
#define ROMAN_ST_TIE_FALLBACK       16  /* top-omega boundary tie: sequential heap emulation ran */
#define ROMAN_ST_INTERNAL           64  /* internal error (a bounded device-side wait of the large-problem solver expired): the
                                           problem has no result; never expected, reported instead of hanging the device */
#define ROMAN_ST_WORKSPACE          32  /* the problem was SKIPPED: roman_align_batch_dev sizes its device pools before the
                                           sizes of the sparse matrices are known (from earlier batches; the call never
                                           waits for the GPU) and this problem did not fit.  The library has recorded the
                                           need: issue the problem again.  The host-pointer and stepwise entry points
                                           retry by themselves and never report this flag. */

/* which invariant scores association pairs */
#define ROMAN_INV_EUCLIDEAN  0  /* clipperpy.invariants.EuclideanDistance + clipperpy.CLIPPER
                                   [REF roman/align/dist_reg_with_pruning.py:48-57]            */
#define ROMAN_INV_ROMAN      1  /* clipperpy.invariants.ROMAN + clipperpy.CLIPPERPairwiseAndSingle
                                   [REF roman/align/roman_registration.py:82-86]               */
#define ROMAN_INV_EUCLIDEAN_PRUNED 2  /* DistRegWithPruning with its NumPy prefilter moved onto the device
                                   [REF roman/align/dist_reg_with_pruning.py:71-97]: EuclideanDistance + clipperpy.CLIPPER on the
                                   associations (i,j) of the all-to-all list that survive
                                       NOT (<desc_i, desc_j> < cosine_min)                       (raw dot product, :75-80)
                                       NOT (min(f_i, f_j) / max(f_i, f_j) < ratio_epsilon[f])    for each of the ratio features (:83-90)
                                   and on ALL of them when none survives (the reference then hands clipperpy an empty list, which
                                   means all-to-all, :94-96).  Feature row: [x y (z)] ++ ratio features (the reference uses volume,
                                   linearity, planarity, scattering) ++ descriptor.  Same result as ROMAN_INV_EUCLIDEAN on the
                                   explicit pruned list (the dot product is accumulated in the order of the f64 matrix core: a
                                   product within rounding of cosine_min may fall on the other side than NumPy's BLAS puts it). */

/* clipperpy.invariants.ROMAN.{GEOMETRIC_MEAN,ARITHMETIC_MEAN,PRODUCT}
   [REF roman/align/roman_registration.py:11-14] */
#define ROMAN_FUSE_GEOMETRIC_MEAN  0
#define ROMAN_FUSE_ARITHMETIC_MEAN 1
#define ROMAN_FUSE_PRODUCT         2

/* The two formulas of the ROMAN invariant that live only in the absent clipperpy sources (SURVEY.md
   Appendix B7, DESIGN.md decisions H2 and H3) are SWITCHES, not hard-wired guesses: 0 is the pinned
   default, the other values are the alternative readings.  The reference never sets them
   ([REF roman/align/roman_registration.py:55-78] lists every attribute it assigns); they exist so that a
   build that can import the real clipperpy can find the reading that reproduces it
   (tests/test_real_clipperpy.py).  With d = displacement between the two objects of a map, h = its
   horizontal length, v = its signed vertical component, l = its full length, unc = gravity_unc_ang_rad:
     ROMAN_GRAV_COMBINED  ch=|h1-h2|, cv=max(0,|v1-v2|-sin(unc)*max(h1,h2)), c=sqrt(ch^2+cv^2); c<epsilon; exp(-c^2/2sigma^2)
     ROMAN_GRAV_SEPARATE  same ch, cv, c; each part gated on its own: ch<epsilon AND cv<epsilon
     ROMAN_GRAV_ZGATE     c=|l1-l2| as for EuclideanDistance, plus the hard gate |v1-v2| < epsilon+sin(unc)*max(l1,l2) */
#define ROMAN_GRAV_COMBINED 0
#define ROMAN_GRAV_SEPARATE 1
#define ROMAN_GRAV_ZGATE    2
/*   ROMAN_SINGLE_BOTH     M_pq = fuse(s_a(p,q), s_o(p), s_o(q)), M_pp = s_o(p)
     ROMAN_SINGLE_OFFDIAG  M_pq fused as above, M_pp = 1 (plain CLIPPER's implicit identity)
     ROMAN_SINGLE_DIAG     M_pq = s_a(p,q), M_pp = s_o(p)
   In these three readings an association whose single score is 0 is removed from the problem (its row and column
   of M and C are empty, its u stays 0).
     ROMAN_SINGLE_DIAG_KEEP  M_pq = s_a(p,q), M_pp = s_o(p) — and NOTHING is removed: an association with s_o = 0 keeps
                             its off-diagonal entries and only has a zero diagonal (SURVEY.md B7 read literally: "diagonal
                             M_pp = s_single(p)", the pair score alone off the diagonal).  Every input association is then
                             live (L = A): the large-live-set path (k_solve_wide) serves it. */
#define ROMAN_SINGLE_BOTH      0
#define ROMAN_SINGLE_OFFDIAG   1
#define ROMAN_SINGLE_DIAG      2
#define ROMAN_SINGLE_DIAG_KEEP 3

/*
 * Invariant + solver parameters.  Replaces clipperpy.invariants.ROMANParams /
 * EuclideanDistanceParams (attributes set at [REF roman/align/roman_registration.py:55-78],
 * [REF roman/align/dist_reg_with_pruning.py:49-52]) and clipperpy.Params (always
 * default-constructed: [REF roman/align/roman_registration.py:84]).
 * roman_params_default() fills the defaults documented in DESIGN.md §"Pinned decisions".
 */
typedef struct roman_params {
    /* invariant */
    int32_t invariant;            /* ROMAN_INV_*                                              */
    int32_t point_dim;            /* 2 or 3                                                   */
    int32_t ratio_feature_dim;    /* <= ROMAN_MAX_RATIO_FEATURES                              */
    int32_t cos_feature_dim;      /* descriptor length d (0 = no semantics)                   */
    int32_t fusion_method;        /* ROMAN_FUSE_*                                             */
    int32_t gravity_guided;       /* 0/1; requires point_dim==3                               */
    int32_t drift_aware;          /* must be 0 (the reference always passes False)            */
    int32_t rescale_u0;           /* clipperpy.Params.rescale_u0 (default 1)                  */
    double  sigma;
    double  epsilon;
    double  mindist;
    double  distance_weight;
    double  ratio_weight;
    double  cosine_weight;
    double  cosine_min;
    double  cosine_max;
    double  gravity_unc_ang_rad;
    double  ratio_epsilon[ROMAN_MAX_RATIO_FEATURES];
    /* solver: clipperpy.Params */
    double  tol_u;                /* 1e-8  */
    double  tol_F;                /* 1e-9  */
    double  beta;                 /* 0.25  */
    double  eps;                  /* 1e-9  */
    double  affinityeps;          /* 1e-4  */
    int32_t maxiniters;           /* 200   */
    int32_t maxoliters;           /* 1000  */
    int32_t maxlsiters;           /* 99    */
    /* decision switches (see ROMAN_GRAV_*, ROMAN_SINGLE_* above); 0 = the pinned default */
    int32_t gravity_mode;         /* ROMAN_GRAV_*   : reading of the gravity-guided pair score (H2)   */
    int32_t single_mode;          /* ROMAN_SINGLE_* : where single scores enter M (H3)                */
    int32_t reserved;             /* must be 0                                                        */
} roman_params_t;

/* per-problem statistics (the quantities SURVEY.md §8(d) builds the roofline from) */
typedef struct roman_stats {
    int32_t n_assoc_in;    /* A: associations scored                                          */
    int32_t n_live;        /* L: associations with a non-zero single score (== A for EUCLIDEAN) */
    int64_t nnz_upper;     /* stored non-zeros of the strict upper triangle of M              */
    int32_t n_pass;        /* sparse matrix-vector passes over M the solver performed         */
    int32_t outer_iters;   /* homotopy (d-update) iterations                                  */
    int32_t inner_iters;   /* accepted projected-gradient steps                               */
    int32_t ls_trials;     /* line-search trials (each is one pass)                           */
    double  score;         /* F = u'Mu at exit (clipper.get_solution().score)                 */
    double  d_final;       /* final homotopy penalty                                          */
} roman_stats_t;

typedef struct roman_ctx roman_ctx_t;

/* ------------------------------------------------------------------------------------------- */
/* library / context                                                                           */
/* ------------------------------------------------------------------------------------------- */

/* Fill *p with the reference defaults: ROMAN invariant, dim 3, sigma .4, epsilon .6,
   mindist .2 [REF roman/params/submap_align_params.py:66-74], weights 1
   [REF roman/align/roman_registration.py:64-66], clipperpy.Params() defaults. */
ROMAN_API int roman_params_default(roman_params_t* p);

/* Create a context bound to HIP device `device`.  `stream` is a hipStream_t passed as void*
   (NULL = the library creates and owns its own non-blocking stream).  The context owns all
   device workspace; it grows on demand and is reused across calls.  One context per
   (device, stream); calls on one context must not overlap.  Replaces the per-call
   `clipperpy.CLIPPER*(invariant, params)` construction of
   [REF roman/align/object_registration.py:25]. */
ROMAN_API int roman_ctx_create(roman_ctx_t** ctx, int device, void* stream);
ROMAN_API int roman_ctx_destroy(roman_ctx_t* ctx);

/* Batches in flight.  depth 1 (default): every call runs on the context's stream and its results are
   complete once that stream is synchronised.  depth 2 ... 6: consecutive roman_align_batch_dev calls rotate
   over that many internal workspaces, each on an internal stream that starts behind the work already queued
   on the context's stream, so the straggler tail of one batch's kernels overlaps the next batch's
   affinity build (the reference's loop [REF roman/align/submap_align.py:93-200] has no dependency
   between pairs).  With depth >= 2 the results of a batch call are complete after roman_ctx_sync() (or a
   device-wide synchronisation), NOT after synchronising the context's stream alone; the caller must give
   batches that may be in flight together distinct output buffers if it needs both results.  The
   host-pointer and stepwise entry points always drain the pipeline first and run synchronously.
   roman_align_batch_dev is a pure enqueue at every depth (it never waits for the device and reads nothing
   back), so one host thread keeps all the batches in flight fed; no library threads exist.  Device buffers
   must stay valid until roman_ctx_sync(). */
ROMAN_API int roman_ctx_set_pipeline(roman_ctx_t* ctx, int depth);
/* Enqueue on the context's stream a wait for the pipelined batches issued so far: all of them, or —
   skip_latest != 0 — all but the most recent one, so that work queued on the caller's stream afterwards
   (e.g. the all_gather of batch k-1's records) sees their results while batch k keeps running.  The host
   does not block. */
ROMAN_API int roman_ctx_join(roman_ctx_t* ctx, int skip_latest);
/* The same wait enqueued on ANOTHER stream of the caller's (a hipStream_t; NULL = the context's stream — NOT the legacy default
   stream, whose handle is also 0: work queued on the null stream cannot be ordered through this call; use an explicit stream): the collective that
   gathers batch k-1's records then runs on a side stream and never sits between two batch calls on the context's stream —
   every batch call starts behind what is queued THERE, so a wait for batch k-1 on it would hold back batch k+1 and cost a
   batch in flight.  The caller orders the reuse of an output buffer against its own side stream (an event). */
ROMAN_API int roman_ctx_join_on(roman_ctx_t* ctx, int skip_latest, void* stream);
/* Wait for every batch in flight on this context (all internal streams and the context's stream). */
ROMAN_API int roman_ctx_sync(roman_ctx_t* ctx);
/* How roman_align_batch (host pointers) issues a LARGE batch: more than `chunk` problems (default 2048) go to the device as
   calls of `chunk` problems with `depth` of them in flight (default 3; 1 = one call for the whole batch, as before round 5) —
   the pipelined loop a device-pointer caller would write around roman_align_batch_dev, done by the library for the caller of
   the reference's serial loop [REF roman/align/submap_align.py:93-200] who hands over every surviving pair at once.  Problems
   a call skipped for workspace are issued again (those only); without a sizing history for the parameter block the first call
   is waited for before the others are queued.  The depth set with roman_ctx_set_pipeline is restored on return. */
ROMAN_API int roman_ctx_set_host_batching(roman_ctx_t* ctx, int chunk, int depth);
/* Team mode of the whole-device solver for LARGE live sets (methods without a semantic gate,
   [REF roman/params/submap_align_params.py:98-116]: every association live): -1 (default) the library decides — several such
   problems in a batch are solved side by side, the workgroups of an XCD (or of half an XCD) on one problem each —, 0 never (the
   whole device on one problem at a time), 1 / 2 / 4 teams per XCD whenever the live sets fit.  Teams are formed on the device
   from the XCD every workgroup really runs on, their buffers are sized on the host from the XCD count the runtime reports: a
   team that cannot hold its problem leaves it ROMAN_ST_INTERNAL; roman_align_batch runs such problems again with teams off, a
   caller of roman_align_batch_dev does the same through this setter. */
ROMAN_API int roman_ctx_set_wide_teams(roman_ctx_t* ctx, int teams_per_xcd);

/* Human-readable text of the last error on this context (or of the last context-less error
   when ctx == NULL).  The pointer stays valid until the next call on the same context. */
ROMAN_API const char* roman_last_error(const roman_ctx_t* ctx);

/* ------------------------------------------------------------------------------------------- */
/* the hot path, batched: score -> solve -> select -> pose for B independent submap pairs      */
/* ------------------------------------------------------------------------------------------- */

/*
 * roman_align_batch_dev: bulk data device-resident.
 *
 * Replaces, for each of the B problems, the reference sequence
 *     clipper.score_pairwise_and_single_consistency(D1, D2, A)   [REF roman/align/roman_registration.py:95]
 *  or clipper.score_pairwise_consistency(D1, D2, A)              [REF roman/align/object_registration.py:47]
 *     clipper.solve()                                            [REF roman/align/object_registration.py:27]
 *     clipper.get_selected_associations()                        [REF roman/align/object_registration.py:28]
 *     ObjectRegistration.T_align(map1, map2, associations)       [REF roman/align/object_registration.py:88-129]
 * i.e. the body of the serial double loop at [REF roman/align/submap_align.py:93-200].
 *
 *   feats      DEVICE, float64: pool of object-major feature matrices (F doubles per object)
 *   off1/off2  HOST, int64[B]: index (in objects) of problem b's first map-1 / map-2 object
 *              in `feats` (several problems may share a submap: the all-pairs grid)
 *   n1/n2      HOST, int32[B]: objects in map 1 / map 2 of problem b
 *   F          features per object = point_dim + ratio_feature_dim + cos_feature_dim
 *   assoc      DEVICE, int32 (sum A_b, 2) or NULL (= all-to-all for every problem)
 *   assoc_off  HOST, int64[B+1] row offsets into assoc (ignored when assoc == NULL), non-decreasing from 0;
 *              a problem whose list is EMPTY is scored all-to-all, as clipperpy does with an empty A
 *              (the reference reaches that case when its prefilter prunes everything,
 *              [REF roman/align/dist_reg_with_pruning.py:94-96]).  Rows must satisfy 0 <= i < n1, 0 <= j < n2:
 *              the host-pointer entry below checks them, this one cannot (device memory) and trusts the caller
 *   u0         DEVICE, float64 initial vectors, concatenated per problem in association order,
 *              or NULL (= all ones; DESIGN.md decision H1)
 *   kmax       capacity (rows) of each problem's slot in assoc_out
 *   assoc_out  DEVICE, int32[B][kmax][2]: selected associations (map-1 index, map-2 index),
 *              in clipperpy order (descending u)
 *   n_assoc_out DEVICE, int32[B]
 *   T_out      DEVICE, float64[B][16]: pose map2->map1, row-major (dim+1)^2 in the leading
 *              entries; NaN-filled when status has ROMAN_ST_INSUFFICIENT/EMPTY_MAP
 *              (the sentinel of [REF roman/align/submap_align.py:179-184])
 *   status_out DEVICE, int32[B]
 *   stats_out  DEVICE, roman_stats_t[B] or NULL
 *
 * The small per-problem metadata arrays are host memory (the library stages them itself);
 * all bulk data stays in HBM.
 * A PURE ENQUEUE: never synchronises a stream, never reads anything back.  The sparse workspace is sized before
 * the live counts are known — from what earlier batches with the same parameter block needed (the totals of a
 * finished batch are picked up from pinned memory without waiting), or from first-call heuristics; the device
 * checks every capacity itself, and a problem that does not fit is SKIPPED: status ROMAN_ST_WORKSPACE, no
 * associations, NaN pose.  Run those problems again (by then the context knows their sizes).  Results are
 * complete once the stream is synchronised (depth 1) / after roman_ctx_sync() (depth >= 2).
 */
ROMAN_API int roman_align_batch_dev(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                          const double* feats, const int64_t* off1, const int32_t* n1,
                          const int64_t* off2, const int32_t* n2, int32_t F,
                          const int32_t* assoc, const int64_t* assoc_off,
                          const double* u0,
                          int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                          double* T_out, int32_t* status_out, roman_stats_t* stats_out);

/* Problems that roman_align_batch_dev calls on this context have reported with ROMAN_ST_WORKSPACE so far (a running
   total; only batches whose totals have arrived count: wait != 0 synchronises every stream of the context first, so
   that all issued batches count).  A caller that never looks at status_out can still tell that something was skipped:
       int64_t before, after;
       roman_ctx_skipped(ctx, 1, &before);
       roman_align_batch_dev(ctx, ...);                          // enqueue (any number of calls)
       roman_ctx_skipped(ctx, 1, &after);                        // waits for them
       if (after != before) { ... status_out[b] & ROMAN_ST_WORKSPACE marks the problems: issue THOSE again — same call
                                  with off1/n1/off2/n2/assoc_off restricted to them; the context has recorded their need,
                                  so the second attempt sizes its pools for them ... }
   roman_align_batch (host pointers) runs exactly this loop itself (at most 5 attempts, then ROMAN_E_NOMEM). */
ROMAN_API int roman_ctx_skipped(roman_ctx_t* ctx, int wait, int64_t* n_skipped);

/* Same contract with HOST pointers everywhere; `n_objects` = number of objects in `feats`.
   Copies in, runs roman_align_batch_dev, copies out, synchronises.  This is what a cgo/ctypes
   binding that holds NumPy arrays calls. */
ROMAN_API int roman_align_batch(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                      const double* feats, int64_t n_objects,
                      const int64_t* off1, const int32_t* n1,
                      const int64_t* off2, const int32_t* n2, int32_t F,
                      const int32_t* assoc, const int64_t* assoc_off,
                      const double* u0,
                      int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                      double* T_out, int32_t* status_out, roman_stats_t* stats_out);

/* Inputs in HBM as for roman_align_batch_dev (feats, assoc, u0: DEVICE pointers; the metadata arrays host memory), results on the
   HOST as for roman_align_batch: what a caller needs whose submaps' feature pool stays resident (the all-pairs grid: every submap
   is uploaded once, [REF roman/align/submap_align.py:93-94]) but who consumes associations and poses on the host
   ([REF roman/align/submap_align.py:155-166]).  Synchronous; chunks, pipelines and retries like roman_align_batch.  The outputs of all
   problems land in one device block and come back with ONE copy through a pinned landing block owned by the context (a single
   pair's whole result — associations, count, pose, status, statistics — is 1.8 KB).  Device buffers must not be in use by work
   queued on streams the context does not know (the call starts behind the context's stream). */
ROMAN_API int roman_align_batch_resident(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                               const double* feats, const int64_t* off1, const int32_t* n1,
                               const int64_t* off2, const int32_t* n2, int32_t F,
                               const int32_t* assoc, const int64_t* assoc_off,
                               const double* u0,
                               int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                               double* T_out, int32_t* status_out, roman_stats_t* stats_out);

/* Does the context hold a sizing history for this parameter block (params, F) — i.e. has a batch with it reported what its sparse
   pools needed?  *yes = 1 / 0.  A device-pointer caller that queues several calls at once asks this first: without a history the
   first call should be waited for (roman_ctx_sync), so that the calls behind it size their pools from what it needed instead of
   repeating its guess (roman_align_batch does the same internally).  The context keeps ONE history: that of the latest block. */
ROMAN_API int roman_ctx_has_history(roman_ctx_t* ctx, const roman_params_t* params, int32_t F, int32_t* yes);

/* The cosine stage of a batch ([REF roman/align/roman_registration.py:52-59]: the semantic similarity only counts above cosine_min) has two
   implementations: the dense f64 matrix-core product of all pairs, and a bf16 screen of all pairs followed by the exact f64 contraction of
   the pairs the screen cannot rule out (k_cos_sel: same bits wherever the gate lets a pair through).  The library picks per batch — large
   batches of maps of at most 256 objects take the screen unless the latest screened batch of the parameter block left more than a quarter of
   its problems to the dense kernel (descriptors that are all alike).  Diagnostics: the numbers of batches that took either since the context
   was created, and the share of the latest screened batch that fell back (any pointer may be NULL).  ROMAN_COS_SEL=0 / 1 forces either. */
ROMAN_API int roman_ctx_cosine_screen_stats(roman_ctx_t* ctx, int64_t* screened_batches, int64_t* dense_batches, double* latest_fallback_share);

/* The deal of a batch over `world` ranks (one process per GPU), for a C / C++ caller that shards with its own collective
   (roman_ros, [REF README.md:11]; the Python side is roman_amd.align.distributed.align_sharded).  The pairs of the serial loop
   [REF roman/align/submap_align.py:93-200] are independent: every rank aligns its share with roman_align_batch[_dev] and ONE
   all_gather of the outputs (n_assoc_out, assoc_out, T_out, status_out: fixed-size rows per problem) collects them — no other
   exchange.  The deal is a pure host function of the problem sizes, identical on every rank without communication: problems
   longest-first (work estimate = the SQUARE of the association count, n1*n2 for all-to-all: pair tests and matrix entries grow
   with it) to the rank with the least work so far, ties to the rank holding fewer problems, then to the lowest rank.
   assoc_off: NULL (all-to-all) or int64[B+1] (an empty list means all-to-all).  idx_out: int32[B] capacity; on return its first
   *n_out entries are the ascending problem indices of `rank`. */
ROMAN_API int roman_deal_problems(int32_t B, const int32_t* n1, const int32_t* n2, const int64_t* assoc_off,
                                  int32_t world, int32_t rank, int32_t* idx_out, int32_t* n_out);

/* ------------------------------------------------------------------------------------------- */
/* loop closures: the tail behind the pose (gravity filters, error metrics, acceptance, edge)  */
/* ------------------------------------------------------------------------------------------- */

/* What the reference does with a pose before it reaches RPGO ([REF roman/align/submap_align.py:160-200],
   [REF roman/align/results.py:156-198]), per problem, on the device.  Flag bits of roman_lc_record_t.flags: */
#define ROMAN_LC_ACCEPTED             1  /* association count >= lc_association_thresh and enabled: the problem is a loop closure,
                                            edge_t / edge_q are set and its index is in the accepted list [REF roman/align/results.py:158-162] */
#define ROMAN_LC_FAILED_INSUFFICIENT  2  /* ROMAN_ST_INSUFFICIENT / ROMAN_ST_EMPTY_MAP: T_align raised [REF roman/align/submap_align.py:179-184] */
#define ROMAN_LC_FAILED_TILT          4  /* roll or pitch of the estimate not below tilt_thresh: GravityConstraintError of the pruning
                                            plugin [REF roman/align/dist_reg_with_pruning.py:38-45] */
#define ROMAN_LC_FAILED_UPSIDE_DOWN   8  /* |roll| or |pitch| above 90 degrees with force_rm_upside_down [REF roman/align/submap_align.py:167-170] */
#define ROMAN_LC_SKIPPED             16  /* ROMAN_ST_WORKSPACE: the batch call skipped the problem; neither failed nor accepted — issue it again */
#define ROMAN_LC_INTERNAL            32  /* ROMAN_ST_INTERNAL: the problem has no result; neither failed nor accepted */

/* The switches of the tail: SubmapAlignParams.force_rm_upside_down / force_rm_lc_roll_pitch
   [REF roman/params/submap_align_params.py:66-74], DistRegWithPruning.roll_pitch_thresh
   [REF roman/align/dist_reg_with_pruning.py:17-27] and SubmapAlignInputOutput.lc_association_thresh
   [REF roman/params/submap_align_params.py:153-198]. */
typedef struct roman_lc_params {
    int32_t dim;                     /* 2 or 3: layout of the poses (row-major (dim+1)^2 in the leading entries of 16 doubles) */
    int32_t force_rm_upside_down;    /* 0/1 (dim 3 only)                                                   */
    int32_t force_rm_lc_roll_pitch;  /* 0/1 (dim 3 only): keep the yaw of the estimate only                */
    int32_t lc_association_thresh;   /* accepted: association count >= this                                */
    double  tilt_thresh;             /* radians; < 0: no tilt check (dim 3 only)                           */
    int32_t reserved[2];             /* must be 0                                                          */
} roman_lc_params_t;

/* One record per problem.  A failed, skipped or internal problem carries the sentinels of
   [REF roman/align/submap_align.py:179-184]: NaN pose, theta 180.0, dist 1e6, no associations. */
typedef struct roman_lc_record {
    int32_t problem;       /* index of the problem in the call                                              */
    int32_t n_assoc;       /* association count after the failure checks (0 when failed)                    */
    int32_t flags;         /* ROMAN_LC_*                                                                    */
    int32_t reserved;      /* 0                                                                             */
    double  T_hat[16];     /* row-major 4x4: the estimate after the post-filters (dim 2: lifted to SE(3))   */
    double  theta;         /* radians: rotation magnitude (dim 3) / signed planar angle (dim 2) of inv(T_hat) T_ref; NaN without T_ref */
    double  dist;          /* norm of the translation of inv(T_hat) T_ref; NaN without T_ref               */
    double  edge_t[3];     /* accepted: translation of FL[iL] T_hat FR[iR]; NaN otherwise                   */
    double  edge_q[4];     /* accepted: its rotation as a quaternion, xyzw, scipy's as_quat() sign: the component picked by the first
                              maximum of (R00, R11, R22, trace) is non-negative, nothing else is normalised; NaN otherwise */
} roman_lc_record_t;

/*
 * roman_lc_tail_dev: the tail on its own, for a caller that holds batch outputs in HBM.  All bulk pointers DEVICE; a pure
 * enqueue on the context's stream (complete once that stream is synchronised).  At pipeline depth >= 2 the batch calls write
 * their outputs on internal streams: order them in front of the tail with roman_ctx_join().
 *
 * Replaces, per problem, pass 2 of the pair loop [REF roman/align/submap_align.py:160-200] (post-filters, error metrics,
 * sentinels) and the edge of save_submap_align_results [REF roman/align/results.py:156-198] (acceptance by association count,
 * composition into the odometry frames, translation + quaternion).
 *
 *   T, n_assoc, status   the outputs of a batch call: float64[B][16], int32[B], int32[B]
 *   T_ref         float64[B][16] row-major 4x4 reference transforms (T_ij of [REF roman/align/submap_align.py:120-127]) or NULL
 *   enable        int32[B] or NULL: a zero entry keeps the problem from being accepted (the single-robot time gate of
 *                 [REF roman/align/results.py:160-162] is evaluated by the caller)
 *   FL, iL        float64[SL][16] per-SUBMAP frames of the left side and int32[B] the submap of each problem, or both NULL
 *                 (identity): what [REF roman/align/results.py:163-169] computes as inv(T_odomi_pi) T_odomi_ci
 *   FR, iR        the same for the right side: inv(T_odomj_cj) T_odomj_pj
 *   records       roman_lc_record_t[B]
 *   accepted_idx  int32[B] capacity: the indices of the accepted problems in ASCENDING order (the order in which the
 *                 reference writes its edges), found by a prefix sum, not by atomics
 *   n_accepted    int32[1]
 */
ROMAN_API int roman_lc_tail_dev(roman_ctx_t* ctx, const roman_lc_params_t* lc_params, int32_t B,
                                const double* T, const int32_t* n_assoc, const int32_t* status,
                                const double* T_ref, const int32_t* enable,
                                const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                                roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted);

/* roman_align_batch_dev followed by the tail over its outputs, enqueued on the SAME stream as that call's solver (the internal
   stream of its workspace at pipeline depth >= 2): the body of the pair loop [REF roman/align/submap_align.py:93-200] and the
   edge of [REF roman/align/results.py:156-198] in one pure enqueue.  Complete after roman_ctx_sync() like the batch call.
   A problem the batch call skipped (ROMAN_ST_WORKSPACE) has a ROMAN_LC_SKIPPED record: issue it again. */
ROMAN_API int roman_align_lc_batch_dev(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                          const double* feats, const int64_t* off1, const int32_t* n1,
                          const int64_t* off2, const int32_t* n2, int32_t F,
                          const int32_t* assoc, const int64_t* assoc_off,
                          const double* u0,
                          int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                          double* T_out, int32_t* status_out, roman_stats_t* stats_out,
                          const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                          const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                          roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted);

/* The same with HOST pointers everywhere (n_left / n_right: submaps in FL / FR): roman_align_batch with its chunking and
   re-issues first, THEN the tail over the final device block — a record is never built from a skipped attempt —, then one
   read-back of outputs, records, index list and count through the pinned landing block.  What the caller of the reference's
   submap_align() + save_submap_align_results() needs ([REF roman/align/submap_align.py:74-220],
   [REF roman/align/results.py:122-198]). */
ROMAN_API int roman_align_lc_batch(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                      const double* feats, int64_t n_objects,
                      const int64_t* off1, const int32_t* n1,
                      const int64_t* off2, const int32_t* n2, int32_t F,
                      const int32_t* assoc, const int64_t* assoc_off,
                      const double* u0,
                      int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                      double* T_out, int32_t* status_out, roman_stats_t* stats_out,
                      const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                      const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                      roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted);

/* ------------------------------------------------------------------------------------------- */
/* self loop closures: segments both submaps of a pair hold are removed first                  */
/* ------------------------------------------------------------------------------------------- */

/*
 * roman_shared_ids_dev: which objects of a pair stay.  For one robot closing loops against its own map
 * (SubmapAlignParams.single_robot_lc) the reference removes from both submaps every segment whose id occurs in both before it
 * registers the pair — the ids of either side as sets, their intersection, and both segment lists without the members of it
 * [REF roman/align/submap_align.py:108-115].  This is that membership test for B pairs over one pool, as a PURE ENQUEUE on the
 * context's stream (complete once that stream is synchronised).
 *
 *   ids        DEVICE, int64: one id per row of the feature pool (full 64-bit equality; an id repeated inside a map is kept or
 *              dropped with all its repetitions)
 *   off1/off2  HOST, int64[B], n1/n2 HOST, int32[B]: the two maps of problem b are ids[off1[b] .. +n1[b]) and
 *              ids[off2[b] .. +n2[b]), as for roman_align_batch_dev (problems may share slices; the two sides may be the same
 *              slice); the call trusts them to lie inside `ids`.  Maps of length 0 and B == 0 are legal
 *   keep       DEVICE, int32[sum over b of (n1[b] + n2[b])]: problem b's side-1 list starts at the sum over c < b of
 *              (n1[c] + n2[c]), its side-2 list n1[b] entries later; each list holds the LOCAL indices (0 .. n-1) of the
 *              objects that stay, ascending, in its first kept[b][side] entries (the rest of the slot is not written)
 *   kept       DEVICE, int32[B][2]: objects that stay on side 1 / side 2
 */
ROMAN_API int roman_shared_ids_dev(roman_ctx_t* ctx, int32_t B, const int64_t* ids,
                                   const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                                   int32_t* keep, int32_t* kept);

/*
 * roman_shared_reduce_dev: the whole removal of [REF roman/align/submap_align.py:108-115] for B pairs over a pool that is
 * ALREADY in HBM — which objects stay (as roman_shared_ids_dev) and the reduced maps themselves — in ONE launch, as a PURE
 * ENQUEUE on the context's stream (complete once that stream is synchronised; nothing is waited for but the previous call's
 * upload of its problem descriptors).  The host needs no count to place anything:
 *
 *   feats      DEVICE, double: the pool's rows (F doubles each), and behind them, from row region_row0 on, a gather region of
 *              sum over b of (n1[b] + n2[b]) rows in the same allocation
 *   ids        DEVICE, int64: one id per pool row
 *   off1/off2  HOST, int64[B], n1/n2 HOST, int32[B]: as for roman_shared_ids_dev; every slice lies in front of the region
 *              (off + n <= region_row0)
 *   keep, kept DEVICE, out: exactly what roman_shared_ids_dev writes
 *
 * With kb[b] = sum over c < b of (n1[c] + n2[c]) (the start of problem b's keep lists), a problem that lost an object on either
 * side (kept[b][0] != n1[b] or kept[b][1] != n2[b]) has its kept rows copied bit for bit, in list order, into FIXED slots:
 * side 1 to rows region_row0 + kb[b] .. + kept[b][0], side 2 to rows region_row0 + kb[b] + n1[b] .. + kept[b][1].  The rows of
 * a slot behind the kept ones are not written, and a problem with kept == n on both sides writes no row at all: it reads the
 * pool as given.  The caller reads `kept` back (8 bytes per problem) and hands the batch calls off = region_row0 + kb (+ n1),
 * n = kept for the problems that lost something and the original off, n for the others; a side reduced to nothing is a map of
 * length 0 (ROMAN_ST_EMPTY_MAP).  The price of placing without counts is memory: the region takes 8 * F * sum (n1 + n2) bytes
 * whatever is lost (roman_align_lc_batch_ids, which reads the counts back first, takes the rows of the affected problems only).
 *
 * ROMAN_E_INVALID (text in roman_last_error; nothing is enqueued): NULL context, B < 0, F < 1, region_row0 < 0, NULL metadata,
 * a negative size or offset, a slice that reaches past region_row0, NULL kept, NULL feats / ids / keep when any map has a row.
 * B == 0 is legal and enqueues nothing.
 */
ROMAN_API int roman_shared_reduce_dev(roman_ctx_t* ctx, int32_t B, int32_t F, double* feats, int64_t region_row0, const int64_t* ids,
                                      const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                                      int32_t* keep, int32_t* kept);

/*
 * roman_align_lc_batch_ids: roman_align_lc_batch (HOST pointers everywhere, same arguments, same results) for pairs that first
 * lose the segments both sides hold — the whole body of the reference's loop for single_robot_lc
 * ([REF roman/align/submap_align.py:108-115] in front of [REF :150-200] and [REF roman/align/results.py:156-198]) with every
 * submap uploaded ONCE instead of one reduced copy per pair.
 *
 *   ids        int64[n_objects]: one id per row of feats
 *   n1_kept, n2_kept   int32[B] out: objects of either side that stayed
 *   keep       int32[sum (n1[b] + n2[b])] out, the layout of roman_shared_ids_dev, or NULL
 *   assoc      must be NULL: explicit lists index the maps before the removal; given together with ids the call returns
 *              ROMAN_E_INVALID (text in roman_last_error)
 *   u0         NULL, or per problem the all-to-all order of the REDUCED maps
 *
 * The pool and the ids are uploaded once; the mark step runs; the kept counts come back (8 bytes per problem, one
 * synchronisation) and size the gather region on the host; k_shared_gather copies the kept rows of the AFFECTED problems
 * (those that lost an object) behind the pool, bit for bit; those problems then read the gather region with their reduced
 * sizes — a side reduced to nothing is a map of length 0: ROMAN_ST_EMPTY_MAP — and the others read the shared pool as
 * given.  From there on the call IS roman_align_lc_batch: chunks, calls in flight, the sizing history, re-issues of skipped
 * problems, the tail after the final attempt only.  Returned associations index the reduced maps, as the reference's do.
 * The extra device memory is the rows of the affected problems; when it cannot be had the call returns ROMAN_E_NOMEM and the
 * context stays usable.
 */
ROMAN_API int roman_align_lc_batch_ids(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                      const double* feats, int64_t n_objects,
                      const int64_t* off1, const int32_t* n1,
                      const int64_t* off2, const int32_t* n2, int32_t F,
                      const int32_t* assoc, const int64_t* assoc_off,
                      const double* u0,
                      int32_t kmax, int32_t* assoc_out, int32_t* n_assoc_out,
                      double* T_out, int32_t* status_out, roman_stats_t* stats_out,
                      const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                      const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                      roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted,
                      const int64_t* ids, int32_t* n1_kept, int32_t* n2_kept, int32_t* keep);

/* ------------------------------------------------------------------------------------------- */
/* multi-solution extraction, batched                                                          */
/* ------------------------------------------------------------------------------------------- */

/* ObjectRegistration.mno_clipper(map1, map2, num_solutions) [REF roman/align/object_registration.py:57-86] for B
   independent submap pairs: score the pair as the batch call does, then num_solutions times — solve, record the
   selected set, zero that set's block of M — without a host round trip between the rounds.  Per problem:
     - every solve is a PLAIN CLIPPER solve ([REF :60] builds CLIPPER(PairwiseInvariant(), Params())) over ALL A input
       associations: strict upper triangles of the scored M and C, unit diagonal, u0 all ones, the solver parameters
       of `params`.  An association whose single score is 0 under the ROMAN invariant stays a node (an isolated one,
       as in the dense matrices get_affinity_matrix() exports).  Solution 0 is therefore register()'s result for the
       invariants without single scores, and in general NOT for ROMAN_INV_ROMAN;
     - a solution's associations are in clipperpy order (descending u, the tie rule of the batch call);
       score = u_s' M u_s / (u_s' u_s) with u_s = u restricted to the selected nodes and M the scored matrix as
       exported, never masked (its diagonal: the single score for ROMAN, 1 otherwise); 0 for an empty selection;
     - before the next solve M[p][q] becomes 0 for all selected p, q; C keeps its pattern (a masked pair is a
       consistent pair of weight 0); masks accumulate;
     - T is the pose of T_align [REF :88-129] on the solution's associations (the reference's loop returns none).
   One record per (problem, solution): */
typedef struct roman_mno_solution {
    int32_t n_assoc;       /* rows of this solution in assoc_out (at most kmax)                                   */
    int32_t status;        /* ROMAN_ST_* of this solution                                                         */
    double  score;         /* Rayleigh quotient on the unmasked M, 0 when the selection is empty                  */
    double  T[16];         /* pose of this hypothesis, row-major (dim+1)^2 in the leading entries; NaN when the
                              status has ROMAN_ST_INSUFFICIENT / ROMAN_ST_EMPTY_MAP / ROMAN_ST_WORKSPACE          */
} roman_mno_solution_t;

#define ROMAN_MNO_MAX_SOLUTIONS   64    /* num_solutions above this: ROMAN_E_INVALID                              */
#define ROMAN_MNO_MAX_ASSOC     3072    /* associations per problem this call serves (the matrix layout whose values
                                           the mask rewrites); a longer list: ROMAN_E_TOO_LARGE                  */

/*
 * roman_mno_batch_dev: bulk data device-resident, arguments as for roman_align_batch_dev (u0 is always all ones).
 *   num_solutions  1 ... ROMAN_MNO_MAX_SOLUTIONS (else ROMAN_E_INVALID)
 *   assoc_out      DEVICE, int32[B][num_solutions][kmax][2]
 *   sol_out        DEVICE, roman_mno_solution_t[B][num_solutions]
 *   stats_out      DEVICE, roman_stats_t[B][num_solutions] or NULL: the statistics of every solve
 * A PURE ENQUEUE like roman_align_batch_dev (same streams, same pipeline rules): all rounds of all problems are queued
 * at once.  A problem that found no workspace is skipped: ROMAN_ST_WORKSPACE on EVERY one of its solutions — issue it
 * again.  An empty map: ROMAN_ST_EMPTY_MAP, num_solutions empty solutions of score 0 with NaN poses.  More selected
 * associations than kmax: ROMAN_ST_ASSOC_TRUNCATED on that solution; score and pose come from the full set.
 * The sizing history of the plain-CLIPPER view is kept apart from the one of the batch call with the same block
 * (the context holds one history: alternating the two calls makes each start from its first-call estimates).
 */
ROMAN_API int roman_mno_batch_dev(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                                  const double* feats, const int64_t* off1, const int32_t* n1,
                                  const int64_t* off2, const int32_t* n2, int32_t F,
                                  const int32_t* assoc, const int64_t* assoc_off,
                                  int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                                  roman_mno_solution_t* sol_out, roman_stats_t* stats_out);

/* The same with HOST pointers everywhere ([REF roman/align/object_registration.py:57-86] for a caller that holds
   NumPy arrays); `n_objects` = number of objects in `feats`.  Synchronous; copies in, issues the batch in calls of the
   host-batching chunk (roman_ctx_set_host_batching) with its depth in flight, issues skipped problems again (those
   only, at most 5 attempts, then ROMAN_E_NOMEM) and brings the three output arrays back. */
ROMAN_API int roman_mno_batch(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                              const double* feats, int64_t n_objects,
                              const int64_t* off1, const int32_t* n1,
                              const int64_t* off2, const int32_t* n2, int32_t F,
                              const int32_t* assoc, const int64_t* assoc_off,
                              int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                              roman_mno_solution_t* sol_out, roman_stats_t* stats_out);

/*
 * roman_mno_lc_tail_dev: the loop-closure tail over K hypotheses per problem — roman_lc_tail_dev for the output of
 * roman_mno_batch_dev.  What the reference does to a pose before it becomes an edge ([REF roman/align/submap_align.py:160-200],
 * [REF roman/align/results.py:156-198]) for every solution of mno_clipper [REF roman/align/object_registration.py:57-86], and
 * the choice among a problem's hypotheses.  All bulk pointers DEVICE; a pure enqueue on the context's stream; at pipeline
 * depth >= 2 order the batch calls in front of it with roman_ctx_join().
 *
 *   sol           roman_mno_solution_t[B][K]: n_assoc, status and T of hypothesis k of problem b
 *   T_ref, enable, FL, iL, FR, iR   as for roman_lc_tail_dev, PER PROBLEM ([B] entries): the K hypotheses of a problem share them
 *   records       roman_lc_record_t[B * K]: record b * K + k is, field for field, what roman_lc_tail_dev writes for that pose
 *                 with the problem's inputs; record.problem = b * K + k
 *   best          int32[B]: the hypothesis the problem's results come from.  Candidates are the hypotheses whose record has none
 *                 of ROMAN_LC_FAILED_*, ROMAN_LC_SKIPPED, ROMAN_LC_INTERNAL; the largest n_assoc wins, the lower k among equals;
 *                 -1 when no hypothesis qualifies (the pair carries the sentinels of [REF roman/align/submap_align.py:179-184]).
 *                 A candidate need not be accepted (too few associations, enable == 0)
 *   accepted_idx  int32[B * K] capacity, n_accepted int32[1]: the accepted records as b * K + k, ASCENDING, by prefix sum
 *   accepted_best_idx  int32[B] capacity, n_accepted_best int32[1]: the problems b whose best hypothesis is accepted, ASCENDING
 *
 * ROMAN_E_INVALID (text in roman_last_error; nothing is enqueued): NULL context, B < 0, K outside 1 ... ROMAN_MNO_MAX_SOLUTIONS,
 * B * K above INT32_MAX, the parameter errors of roman_lc_tail_dev, a frame pool without its index array, NULL n_accepted /
 * n_accepted_best, and with B > 0 NULL sol / records / best / accepted_idx / accepted_best_idx.  B == 0 is legal: both counts
 * become 0.  Entries of the lists beyond the counts are not written.
 */
ROMAN_API int roman_mno_lc_tail_dev(roman_ctx_t* ctx, const roman_lc_params_t* lc_params, int32_t B, int32_t K,
                                    const roman_mno_solution_t* sol, const double* T_ref, const int32_t* enable,
                                    const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                                    roman_lc_record_t* records, int32_t* best, int32_t* accepted_idx, int32_t* n_accepted,
                                    int32_t* accepted_best_idx, int32_t* n_accepted_best);

/* roman_mno_batch_dev followed by roman_mno_lc_tail_dev over its solutions, enqueued on the SAME stream as that call's rounds
   (the relation of roman_align_lc_batch_dev to roman_align_batch_dev): [REF roman/align/object_registration.py:57-86] and the
   tail of [REF roman/align/submap_align.py:160-200] / [REF roman/align/results.py:156-198] in one pure enqueue, complete after
   roman_ctx_sync().  A problem skipped for workspace has ROMAN_LC_SKIPPED on all K records and best = -1: issue it again. */
ROMAN_API int roman_mno_lc_batch_dev(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                                     const double* feats, const int64_t* off1, const int32_t* n1,
                                     const int64_t* off2, const int32_t* n2, int32_t F,
                                     const int32_t* assoc, const int64_t* assoc_off,
                                     int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                                     roman_mno_solution_t* sol_out, roman_stats_t* stats_out,
                                     const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                                     const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                                     roman_lc_record_t* records, int32_t* best, int32_t* accepted_idx, int32_t* n_accepted,
                                     int32_t* accepted_best_idx, int32_t* n_accepted_best);

/* The same with HOST pointers everywhere (n_left / n_right: submaps in FL / FR): roman_mno_batch with its chunking and
   re-issues first, THEN the tail over the final device block — a record is never built from a skipped attempt —, then the
   read-back (the list entries beyond the counts come back unspecified here: the untouched-slot guarantee is the _dev entries').
   mno_clipper [REF roman/align/object_registration.py:57-86] plus [REF roman/align/submap_align.py:160-200] and
   [REF roman/align/results.py:156-198] per hypothesis for a caller that holds NumPy arrays. */
ROMAN_API int roman_mno_lc_batch(roman_ctx_t* ctx, const roman_params_t* params, int32_t B,
                                 const double* feats, int64_t n_objects,
                                 const int64_t* off1, const int32_t* n1,
                                 const int64_t* off2, const int32_t* n2, int32_t F,
                                 const int32_t* assoc, const int64_t* assoc_off,
                                 int32_t num_solutions, int32_t kmax, int32_t* assoc_out,
                                 roman_mno_solution_t* sol_out, roman_stats_t* stats_out,
                                 const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                                 const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                                 roman_lc_record_t* records, int32_t* best, int32_t* accepted_idx, int32_t* n_accepted,
                                 int32_t* accepted_best_idx, int32_t* n_accepted_best);

/* ------------------------------------------------------------------------------------------- */
/* RANSAC registration on object centres, batched (method 'ransac')                            */
/* ------------------------------------------------------------------------------------------- */

/* RansacReg.register(map1, map2) [REF roman/align/ransac_reg.py:16-53] for B independent submap pairs, with the pose of the
   inherited T_align [REF roman/align/object_registration.py:88-129] on the result.  The reference hands the object centres and
   all n1*n2 correspondences (i, j), row-major, to open3d's registration_ransac_based_on_correspondence (ransac_n 3, an
   edge-length checker, max_correspondence_distance 0.5, confidence 0.999).  open3d samples from a thread-local generator and
   stops on thread timing, so its result cannot be reproduced; this call runs a DETERMINISTIC procedure with the same
   ingredients (DESIGN.md §4.7 is the contract).  Per problem, P = the n1 centres of map 1 (source), Q = the n2 of map 2 (target):
     - hypothesis h takes the correspondences a_k = mulhi64(draw(3h + k), n1*n2), k = 0, 1, 2, (i_k, j_k) = (a_k / n2, a_k % n2);
       draw(c) is output c + 1 of splitmix64 seeded with `seed` (the same seed for every problem of a batch);
     - DEVIATION: a hypothesis two of whose correspondences share a source or a target index is dropped (open3d lets such
       zero-edge triples through its checker).  Otherwise open3d's edge-length check: for each of the three index pairs, with
       ds = |P[i_k] - P[i_l]|, dt = |Q[j_k] - Q[j_l]|, dropped when ds < dt * edge_len or dt < ds * edge_len;
     - the rigid transform source -> target of the three pairs is the library's Kabsch fit (the arithmetic of T_align);
     - every correspondence (i, j) with d2 = |R P[i] + t - Q[j]|^2 < max_dist^2 is an inlier; key = (count, sum of d2 over the
       inliers in row-major order); higher count wins, then lower sum, then lower h (open3d's IsBetterRANSACThan made total);
     - DEVIATION: hypotheses are processed in rounds of `round` consecutive indices and the early stop is decided after whole
       rounds only: with f = best count / (n1*n2), K = max_iteration when f = 0 (or when log(1 - f^3) rounds to 0), 0 when
       f = 1, else min(max_iteration, ceil(log(1 - confidence) / log(1 - f^3))); the problem stops once the hypotheses
       processed reach K or max_iteration (the last round is cut there).  The result is a function of the inputs alone;
     - the winner's inliers go out as (i, j) rows in row-major order (open3d's correspondence_set), the pose is Arun's fit on
       exactly those rows, map 2 -> map 1. */
typedef struct roman_ransac_params {
    int64_t  max_iteration;   /* >= 1: RansacReg.max_iteration [REF roman/align/ransac_reg.py:10,50]                         */
    int32_t  round;           /* >= 1: hypotheses between two evaluations of the stop rule                                   */
    double   edge_len;        /* (0, 1]: RansacReg.edge_len [REF roman/align/ransac_reg.py:49]                               */
    double   max_dist;        /* > 0: max_correspondence_distance [REF roman/align/ransac_reg.py:47]                         */
    double   confidence;      /* (0, 1): open3d's RANSACConvergenceCriteria.confidence (0.999)                               */
    uint64_t seed;
} roman_ransac_params_t;

typedef struct roman_ransac_record {
    int32_t n_assoc;          /* inliers of the winner (the FULL count, also when assoc_out holds only kmax of them)          */
    int32_t status;           /* ROMAN_ST_OK / EMPTY_MAP / INSUFFICIENT (no surviving hypothesis, or fewer than 3 inliers) / ASSOC_TRUNCATED */
    int64_t n_hyp;            /* hypotheses processed                                                                        */
    int64_t n_scored;         /* ... of which survived the prune                                                             */
    int64_t best_hyp;         /* index of the winner; -1: none                                                               */
    int32_t best_count;       /* its inlier count                                                                            */
    double  best_sse;         /* its sum of squared inlier distances                                                         */
    double  T[16];            /* pose map 2 -> map 1, row-major 4x4; NaN with ROMAN_ST_INSUFFICIENT / ROMAN_ST_EMPTY_MAP     */
} roman_ransac_record_t;

#define ROMAN_RANSAC_MAX_OBJECTS 1024   /* objects per side (both point sets of a problem stay in LDS: 48 KB); more: ROMAN_E_TOO_LARGE */

/*
 * roman_ransac_batch_dev [REF roman/align/ransac_reg.py:16-53]: bulk data device-resident; a PURE ENQUEUE on the context's
 * stream (at every pipeline depth), complete once that stream is synchronised.  One workgroup per problem runs all rounds.
 *   pts        DEVICE, float64: pool of object centres, 3 doubles per object (dim 3 only, as the reference asserts)
 *   off1/off2  HOST, int64[B], n1/n2 HOST, int32[B]: as for roman_align_batch_dev (trusted to lie inside `pts`)
 *   kmax       capacity (rows) of each problem's slot in assoc_out
 *   assoc_out  DEVICE, int32[B][kmax][2]: the winner's inliers, row-major order; more inliers than kmax:
 *              ROMAN_ST_ASSOC_TRUNCATED, the first kmax rows, n_assoc / key / pose from the full set
 *   rec_out    DEVICE, roman_ransac_record_t[B]
 *   counts_out DEVICE, int32[B][max_iteration] or NULL: the inlier count of every processed hypothesis, -1 for a pruned one;
 *              untouched beyond n_hyp (one extra store per hypothesis: how the tests see inside)
 * Errors: max_iteration < 1, round < 1, edge_len outside (0, 1], max_dist <= 0, confidence outside (0, 1) -> ROMAN_E_INVALID;
 * a side above ROMAN_RANSAC_MAX_OBJECTS -> ROMAN_E_TOO_LARGE.  An empty map: ROMAN_ST_EMPTY_MAP, no rows, NaN pose.
 */
ROMAN_API int roman_ransac_batch_dev(roman_ctx_t* ctx, const roman_ransac_params_t* rparams, int32_t B,
                                     const double* pts, const int64_t* off1, const int32_t* n1,
                                     const int64_t* off2, const int32_t* n2,
                                     int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out);

/* The same with HOST pointers everywhere ([REF roman/align/ransac_reg.py:16-53] for a caller that holds NumPy arrays);
   `n_objects` = number of objects in `pts`.  Synchronous; the batch is issued in calls of the host-batching chunk
   (roman_ctx_set_host_batching), all on the context's stream. */
ROMAN_API int roman_ransac_batch(roman_ctx_t* ctx, const roman_ransac_params_t* rparams, int32_t B,
                                 const double* pts, int64_t n_objects, const int64_t* off1, const int32_t* n1,
                                 const int64_t* off2, const int32_t* n2,
                                 int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out);

/*
 * RANSAC loop closures: RansacReg.register + T_align [REF roman/align/ransac_reg.py:16-53] for B pairs whose
 * centres lie in a pool of F-double ROWS — a submap pool built for any registration: columns 0-2 of a row are the centre, no
 * other column is read —, pass 2 of the pair loop [REF roman/align/submap_align.py:160-200] and the loop-closure edge
 * [REF roman/align/results.py:156-198] behind it: the baseline of the paper over the pools the ROMAN run uses, in one call.
 *   rows       float64, rows of F >= 3 doubles; problem b reads rows off1[b] .. +n1[b] and off2[b] .. +n2[b] (F = 3: the packed
 *              pool of roman_ransac_batch_dev, which is this kernel with F = 3 and no split outputs)
 *   kmax, assoc_out, rec_out, counts_out   as for roman_ransac_batch_dev
 *   T_out, n_assoc_out, status_out   float64[B][16], int32[B], int32[B], each or NULL: exactly the record's T (NaN with
 *              ROMAN_ST_INSUFFICIENT / ROMAN_ST_EMPTY_MAP), n_assoc (the FULL inlier count, also under ROMAN_ST_ASSOC_TRUNCATED)
 *              and status — what roman_lc_tail_dev reads; required when lc_params is given
 *   lc_params  NULL: no tail, the arguments behind it are ignored.  Otherwise roman_lc_tail_dev's arguments and contract, to
 *              the byte (ROMAN_ST_INSUFFICIENT / ROMAN_ST_EMPTY_MAP -> ROMAN_LC_FAILED_INSUFFICIENT with the sentinels;
 *              tilt_thresh honoured as given); dim must be 3
 * Errors (nothing is enqueued): everything roman_ransac_batch_dev rejects, F < 3, a NULL split output with lc_params,
 * lc_params->dim != 3, non-zero reserved words, FL without iL (FR without iR) or the reverse -> ROMAN_E_INVALID; a side above
 * ROMAN_RANSAC_MAX_OBJECTS -> ROMAN_E_TOO_LARGE.  B == 0 is legal and writes n_accepted = 0 when a tail is asked for.
 */

/* DEVICE bulk pointers; pure enqueue on the context's stream: k_ransac over strided rows, then k_lc_tail + k_lc_compact
   behind it on the same stream (RANSAC never runs on the pipeline's internal streams: no roman_ctx_join needed).
   [REF roman/align/ransac_reg.py:16-53], [REF roman/align/submap_align.py:160-200], [REF roman/align/results.py:156-198] */
ROMAN_API int roman_ransac_lc_batch_dev(roman_ctx_t* ctx, const roman_ransac_params_t* rparams, int32_t B,
                                        const double* rows, int32_t F, const int64_t* off1, const int32_t* n1,
                                        const int64_t* off2, const int32_t* n2,   /* metadata HOST */
                                        int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out /* or NULL */,
                                        double* T_out, int32_t* n_assoc_out, int32_t* status_out,
                                        const roman_lc_params_t* lc_params /* NULL: no tail and the lc arguments are ignored */,
                                        const double* T_ref, const int32_t* enable,
                                        const double* FL, const int32_t* iL, const double* FR, const int32_t* iR,
                                        roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted);

/* The same with HOST pointers everywhere (n_objects rows of F doubles; n_left / n_right submaps in FL / FR): staged through
   the context's one HostMirror block like roman_ransac_batch, issued in calls of the host-batching chunk on the context's
   stream, the tail ONCE over the whole batch behind the last chunk, one read-back.  iL / iR are range-checked here.
   [REF roman/align/ransac_reg.py:16-53], [REF roman/align/submap_align.py:160-200], [REF roman/align/results.py:156-198] */
ROMAN_API int roman_ransac_lc_batch(roman_ctx_t* ctx, const roman_ransac_params_t* rparams, int32_t B,
                                    const double* rows, int64_t n_objects, int32_t F, const int64_t* off1, const int32_t* n1,
                                    const int64_t* off2, const int32_t* n2,
                                    int32_t kmax, int32_t* assoc_out, roman_ransac_record_t* rec_out, int32_t* counts_out,
                                    double* T_out, int32_t* n_assoc_out, int32_t* status_out,
                                    const roman_lc_params_t* lc_params, const double* T_ref, const int32_t* enable,
                                    const double* FL, int32_t n_left, const int32_t* iL, const double* FR, int32_t n_right, const int32_t* iR,
                                    roman_lc_record_t* records, int32_t* accepted_idx, int32_t* n_accepted);

/* ------------------------------------------------------------------------------------------- */
/* submaps from a whole map: slice, prune, pack (radius mode)                                  */
/* ------------------------------------------------------------------------------------------- */

/* The radius mode of submaps_from_roman_map [REF roman/map/map.py:297-339] (force_fill_submaps=False) for the S submap
   centres of one map, on the device: which of the N map segments belong to each submap, in which order, and their feature
   rows in the submap's gravity-aligned frame — the feature pool the batch calls consume, in fixed slots of `cap` rows per
   submap (submap s owns rows [s*cap, s*cap + count[s])), so offsets are known before the call.  DESIGN.md §4.8 is the contract.
   The centres themselves come from a sequential scan of the trajectory [REF :300-309], which stays on the host
   (roman_amd.align.submaps.submap_centers).  The force_fill_submaps mode [REF :264-295] (slices of a time-sorted list) orders
   its slices on the host too (roman_amd.align.submaps.fill_centers) and gathers them with roman_submaps_fill_dev below.
   The frame-descriptor modes of submap_descriptor [REF :348-355] run behind this call on the same stream: roman_frame_select_dev
   below reads the count and src it wrote. */
typedef struct roman_submap_params {
    int32_t point_dim;       /* 2 or 3: leading centre components an output row keeps (the input row always carries x y z)        */
    int32_t max_size;        /* SubmapParams.max_size [REF roman/map/map.py:332-339]; <= 0: None (no sort, rows in map order)     */
    int32_t cap;             /* rows per submap slot, >= 1; must equal max_size when max_size > 0                                 */
    int32_t prune_by_time;   /* pruning_method == 'time' [REF :333-334]; 0: distance [REF :335-336]; read only with max_size > 0  */
    int32_t use_radius;      /* 0: SubmapParams.radius is None [REF :323]                                                         */
    int32_t reserved0;       /* must be 0                                                                                         */
    double  radius;          /* SubmapParams.radius (read only with use_radius)                                                   */
    int32_t reserved[2];     /* must be 0                                                                                         */
} roman_submap_params_t;

/* One submap centre, prepared by the host (S is small) */
typedef struct roman_submap_desc {
    double pos[3];             /* pose_flu[:3,3], the centre the radius test measures from [REF roman/map/map.py:324]             */
    double T_center_odom[16];  /* row-major 4x4 inv(pose_gravity_aligned) [REF :328-330]                                          */
    double time;               /* the submap's time (key of the time pruning [REF :334])                                          */
    double t_hi;               /* next submap's time + time_threshold, +inf for the last submap [REF :316-318]                    */
    double t_lo;               /* previous submap's time - time_threshold, -inf for the first [REF :315,319]                      */
} roman_submap_desc_t;

/*
 * roman_submaps_dev: bulk pointers DEVICE, the descriptors HOST (the library stages them).  A PURE ENQUEUE on the context's
 * stream, complete once that stream is synchronised.  S == 0 and N == 0 are legal.
 *   seg_feats  float64[N][F]: one row per map segment in map order, odom frame: [x y z | ratio features | descriptor]
 *   seg_times  float64[N][2]: first_seen, last_seen
 *   seg_ids    int64[N] or NULL
 *   Segment k belongs to submap s when  (no radius, or sqrt(((cx-px)^2 + (cy-py)^2) + (cz-pz)^2) < radius)  and
 *   NOT (first_seen > t_hi OR last_seen < t_lo) [REF :317-326].  Its centre becomes c' = R c + t of T_center_odom, each component
 *   ((r0 x + r1 y) + r2 z) + t, without fused multiply-adds; every other column is copied bit for bit.  With max_size set the rows
 *   are ordered by ascending key — |c'| (distance pruning) or |(first_seen + last_seen) / 2 - time| (time pruning) —, ties by
 *   ascending map index (Python's stable sorted() [REF :338]), and cut to max_size; the sort happens also when fewer qualify.
 *   Without max_size the rows stay in map order and a submap with more than `cap` members keeps the first `cap` and reports
 *   ROMAN_ST_ASSOC_TRUNCATED.  Keys must not be NaN (one that is sorts as +inf).
 *   pool       float64[S*cap][point_dim + F - 3]; rows beyond count[s] in a slot are not written
 *   count      int32[S]: rows of each submap (0: the reference drops such a submap afterwards [REF :341]; so does the Python layer)
 *   src        int32[S*cap]: map index of every row
 *   ids_out    int64[S*cap] or NULL (needs seg_ids)
 *   status     int32[S]: ROMAN_ST_OK / ROMAN_ST_ASSOC_TRUNCATED
 *   desc_dim, desc_out   float64[S][desc_dim] or NULL: submap_descriptor 'mean_semantic' [REF :343-346] — the LAST desc_dim columns
 *              of the rows, added in output order, divided by the count; untouched for an empty submap
 * A submap's candidates beyond the first 4096 go through a per-submap scratch the context owns (S * (N - 4096) entries of 12 bytes).
 * Errors: bad dims (point_dim, F < 3, N / S < 0, desc_dim outside [0, F - 3]), cap < 1, cap != max_size > 0, reserved words not 0,
 * a NULL pointer that is needed -> ROMAN_E_INVALID; a scratch allocation that fails -> ROMAN_E_NOMEM, the context stays usable.
 */
ROMAN_API int roman_submaps_dev(roman_ctx_t* ctx, const roman_submap_params_t* sparams, int32_t N, int32_t F,
                                const double* seg_feats, const double* seg_times, const int64_t* seg_ids,
                                int32_t S, const roman_submap_desc_t* descs,
                                double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status,
                                int32_t desc_dim, double* desc_out);

/* The same with HOST pointers everywhere ([REF roman/map/map.py:297-346] for a caller that holds NumPy arrays).  Synchronous:
   copies in, runs roman_submaps_dev, brings count, src, ids_out, status, desc_out and — pool != NULL — the pool back.  The
   caller's src, ids_out, desc_out and pool go up first: what the device call leaves untouched comes back as it was. */
ROMAN_API int roman_submaps(roman_ctx_t* ctx, const roman_submap_params_t* sparams, int32_t N, int32_t F,
                            const double* seg_feats, const double* seg_times, const int64_t* seg_ids,
                            int32_t S, const roman_submap_desc_t* descs,
                            double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status,
                            int32_t desc_dim, double* desc_out);

/*
 * roman_session_submaps_dev: roman_submaps_dev [REF roman/map/map.py:297-346] for the R maps of a multi-robot
 * session in ONE launch sequence, straight into the one pool the session's batch reads.  Bulk pointers DEVICE; the offset tables and
 * the descriptors HOST (the library stages what the device needs).  A PURE ENQUEUE on the context's stream.  One parameter block
 * serves every map (one `cap`); radius mode only, use_radius = 0 and max_size <= 0 included.
 *   R, seg_off int64[R+1] HOST: map r owns the segment rows [seg_off[r], seg_off[r+1]) of seg_feats / seg_times / seg_ids, the R map
 *              tables concatenated in map order (N_r = seg_off[r+1] - seg_off[r]); seg_off[0] = 0
 *   sub_off    int32[R+1] HOST: map r owns the submaps [sub_off[r], sub_off[r+1]) (S_r of them); sub_off[0] = 0
 *   descs      roman_submap_desc_t[sub_off[R]] HOST, the maps' centres in map order
 *   pool, count, src, ids_out, status, desc_dim, desc_out   as for roman_submaps_dev, over all sub_off[R] submaps: submap
 *              g = sub_off[r] + s owns the pool rows [g*cap, g*cap + count[g]); src holds MAP-LOCAL indices (0 .. N_r - 1)
 * For every r the slice [sub_off[r], sub_off[r+1]) of count, status and desc_out and the slice [sub_off[r]*cap, sub_off[r+1]*cap) of
 * pool, src and ids_out are BIT FOR BIT what roman_submaps_dev(ctx, sparams, N_r, F, <map r's tables>, S_r, <its descs>, ...) writes;
 * rows beyond count[g] and the descriptor of an empty submap are not written.  R == 0, maps with N_r == 0 and maps with S_r == 0 are
 * legal.  Candidates beyond the first 4096 of a submap go through a scratch the context owns: sum over r of S_r * max(N_r - 4096, 0)
 * entries of 12 bytes, every submap's slice at an offset the host computes; allocated only when some N_r > 4096.
 * Errors: those of roman_submaps_dev; R < 0, a NULL offset table with R > 0, seg_off[0] or sub_off[0] not 0, an offset table that
 * decreases -> ROMAN_E_INVALID; sub_off[R] * cap beyond int32 (or a map of more than 2^31 - 1 rows) -> ROMAN_E_TOO_LARGE; a scratch
 * allocation that fails -> ROMAN_E_NOMEM, nothing is enqueued and the context stays usable.  The arguments are judged before the
 * context: with ctx NULL a refused call answers with its own code.
 */
ROMAN_API int roman_session_submaps_dev(roman_ctx_t* ctx, const roman_submap_params_t* sparams, int32_t R, int32_t F,
                                        const int64_t* seg_off, const double* seg_feats, const double* seg_times, const int64_t* seg_ids,
                                        const int32_t* sub_off, const roman_submap_desc_t* descs,
                                        double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status,
                                        int32_t desc_dim, double* desc_out);

/* The same with HOST pointers everywhere.  Synchronous: copies in, runs roman_session_submaps_dev, brings count, src, ids_out,
   status, desc_out and — pool != NULL — the pool back; what the device call leaves untouched comes back as it was. */
ROMAN_API int roman_session_submaps(roman_ctx_t* ctx, const roman_submap_params_t* sparams, int32_t R, int32_t F,
                                    const int64_t* seg_off, const double* seg_feats, const double* seg_times, const int64_t* seg_ids,
                                    const int32_t* sub_off, const roman_submap_desc_t* descs,
                                    double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status,
                                    int32_t desc_dim, double* desc_out);

/*
 * roman_session_submaps_list_dev: roman_session_submaps_dev [REF roman/map/map.py:297-346] for the L LISTED submaps
 * of a session that grows, rebuilt IN PLACE in outputs that stay in HBM between steps, with a report of which slots changed.  The
 * first 17 arguments are those of roman_session_submaps_dev, over the whole session as it stands now; then
 *   L, list    int32[L] HOST: global submap indices g, strictly ascending, each in [0, sub_off[R])
 *   changed    int32[L] DEVICE or NULL
 * A PURE ENQUEUE on the context's stream.
 * LISTED slots: count[g], status[g], the rows [0, count[g]) of pool, src and ids_out and the desc_out row hold bit for bit what
 * roman_session_submaps_dev writes there for the same inputs (the same per-submap code).  A submap may shrink, so a listed slot is
 * left WHOLE: its rows [count[g], cap) are set to pool 0.0, src -1, ids_out -1 — the values roman_amd's build_session_pools clears its
 * tensors to —, and the desc_out row of an EMPTY listed submap is set to NaN (0x7ff8000000000000) in every column.
 * UNLISTED slots: not one byte is written (or read).
 * changed[l] = 1 when any byte of slot list[l] — count, status, the cap rows of src, ids_out and pool, the desc_out row — differs from
 * what the slot held when the call began, else 0; every flag is one workgroup's reduction and one store, independent of any order.
 * With changed NULL nothing is compared (and the old contents are not read).
 * Candidates beyond the first 4096 of a submap take scratch for the LISTED submaps of maps with N_r > 4096 only.  Every allocation
 * and staging is made before the first copy: a failure -> ROMAN_E_NOMEM, nothing is enqueued and the context stays usable.
 * L == 0 is legal and touches nothing; R == 0, maps without rows and maps without centres stay legal.
 * Errors (judged on host memory before the context): those of roman_session_submaps_dev; L < 0, a NULL list with L > 0, an entry
 * outside [0, sub_off[R]), a list that is not strictly ascending -> ROMAN_E_INVALID.
 */
ROMAN_API int roman_session_submaps_list_dev(roman_ctx_t* ctx, const roman_submap_params_t* sparams, int32_t R, int32_t F,
                                             const int64_t* seg_off, const double* seg_feats, const double* seg_times, const int64_t* seg_ids,
                                             const int32_t* sub_off, const roman_submap_desc_t* descs,
                                             double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status,
                                             int32_t desc_dim, double* desc_out,
                                             int32_t L, const int32_t* list, int32_t* changed);

/* The same with HOST pointers everywhere [REF roman/map/map.py:297-346].  Synchronous: the caller's CURRENT pool, count, src, ids_out,
   status and desc_out go up first (pool is needed here: it is what `changed` compares with), roman_session_submaps_list_dev runs, and
   everything comes back, `changed` (int32[L] or NULL) included: an unlisted slot comes back as it was. */
ROMAN_API int roman_session_submaps_list(roman_ctx_t* ctx, const roman_submap_params_t* sparams, int32_t R, int32_t F,
                                         const int64_t* seg_off, const double* seg_feats, const double* seg_times, const int64_t* seg_ids,
                                         const int32_t* sub_off, const roman_submap_desc_t* descs,
                                         double* pool, int32_t* count, int32_t* src, int64_t* ids_out, int32_t* status,
                                         int32_t desc_dim, double* desc_out,
                                         int32_t L, const int32_t* list, int32_t* changed);

/* ------------------------------------------------------------------------------------------- */
/* frame descriptors of the submaps of a pool                                                  */
/* ------------------------------------------------------------------------------------------- */

/* extract_submap_descriptors [REF roman/map/map.py:210-242] for all S submaps of one pool in one enqueue: which of the map's Nf
   frames every submap holds ('stacked_frame_descriptors', with and without frame_descriptor_dist) and their mean
   ('mean_frame_descriptor').  DESIGN.md §4.10 is the contract. */
typedef struct roman_frame_select_params {
    int32_t thin;            /* 0/1: SubmapParams.frame_descriptor_dist is set [REF roman/map/map.py:226-242]                     */
    int32_t want_mean;       /* 0/1: write `mean` [REF :216-219]                                                                  */
    double  thin_dist;       /* frame_descriptor_dist (read only with thin); NaN or < 0: ROMAN_E_INVALID                          */
    int32_t reserved[2];     /* must be 0                                                                                         */
} roman_frame_select_params_t;

/*
 * roman_frame_select_dev: every pointer DEVICE; a PURE ENQUEUE on the context's stream, complete once that stream is synchronised.
 *   count      int32[S], src int32[S*cap]: as roman_submaps_dev wrote them (rows [s*cap, s*cap + count[s]) are map indices < N)
 *   seg_times  float64[N][2]: first_seen, last_seen of the map table
 *   frame_times float64[Nf]; frame_pos float64[Nf][3] (trajectory pose[:3,3]; read only with thin, may be NULL without);
 *   frame_desc float64[Nf][d] (read only with want_mean, may be NULL without)
 * Per submap s: span[s] = (min first_seen, max last_seen) over the rows the submap keeps — after the prune, as Submap.first_seen /
 * last_seen read them [REF :125-131]; frame f is a candidate when span lo <= frame_times[f] <= span hi [REF :218]; frame order is
 * index order, times need not be sorted.  Without thin every candidate is selected.  With thin the candidates are walked in
 * ascending index: the first is selected, each later one when sqrt((dx^2 + dy^2) + dz^2) to the LAST SELECTED candidate is
 * >= thin_dist [REF :236-240] (no fused multiply-adds).
 *   mask       uint64[S][W], W = ceil(Nf / 64): bit f % 64 of word f / 64; whole words are written, zero where nothing is selected
 *   n_sel      int32[S]
 *   span       float64[S][2]; an empty submap (count 0): n_sel 0, span (+inf, -inf)
 *   mean       float64[S][d] with want_mean: the selected rows added in ascending frame index, then divided by n_sel
 *              (descriptors_np[frame_mask].mean(axis=0) [REF :219]); a fixed order: two calls agree bit for bit; 0 / 0 = NaN for n_sel 0
 * S == 0 and Nf == 0 are legal.  Errors: a NULL pointer that is needed, negative sizes, cap < 1, thin_dist NaN or < 0 with thin,
 * want_mean with d < 1 or frame_desc NULL, reserved words not 0 -> ROMAN_E_INVALID.
 */
ROMAN_API int roman_frame_select_dev(roman_ctx_t* ctx, const roman_frame_select_params_t* fparams, int32_t S, int32_t cap,
                                     const int32_t* count, const int32_t* src, int32_t N, const double* seg_times,
                                     int32_t Nf, const double* frame_times, const double* frame_pos, int32_t d, const double* frame_desc,
                                     uint64_t* mask, int32_t* n_sel, double* span, double* mean);

/* The same with HOST pointers everywhere.  Synchronous: copies in, runs roman_frame_select_dev, brings mask, n_sel, span and mean back. */
ROMAN_API int roman_frame_select(roman_ctx_t* ctx, const roman_frame_select_params_t* fparams, int32_t S, int32_t cap,
                                 const int32_t* count, const int32_t* src, int32_t N, const double* seg_times,
                                 int32_t Nf, const double* frame_times, const double* frame_pos, int32_t d, const double* frame_desc,
                                 uint64_t* mask, int32_t* n_sel, double* span, double* mean);

/* One robot of a session whose frame tables stay in HBM (roman_session_frame_select_list*): its ranges of the session's tensors. */
typedef struct roman_session_frame_robot {
    int64_t seg0;            /* first row of its segment table in seg_times                                                        */
    int64_t mask_off;        /* word offset of its first mask row in `mask`                                                        */
    int32_t n_seg;           /* rows of its segment table (src holds indices < n_seg, local to the robot)                          */
    int32_t sub0;            /* its first global slot                                                                              */
    int32_t n_sub;           /* its slots: [sub0, sub0 + n_sub)                                                                    */
    int32_t frame0;          /* its first frame in frame_times / frame_pos / frame_desc                                            */
    int32_t n_frames;        /* Nf_r                                                                                               */
    int32_t mask_words;      /* words per mask row, a CAPACITY: >= ceil(Nf_r / 64)                                                 */
    int32_t reserved[2];     /* must be 0                                                                                          */
} roman_session_frame_robot_t;

/*
 * roman_session_frame_select_list_dev: roman_frame_select_dev [REF roman/map/map.py:210-242] for the L LISTED slots
 * of a session that grows, IN PLACE in outputs that stay in HBM between steps, with a report of which slots changed.  Bulk pointers
 * DEVICE; `robots` and `list` HOST (the library stages them); a PURE ENQUEUE on the context's stream.
 *   robots     roman_session_frame_robot_t[R]: segment rows, slots, frames and mask rows of every robot; each kind of range
 *              ascending and disjoint over the robots (robot r + 1 starts at or behind the end of robot r)
 *   count      int32[S], src int32[S*cap], by GLOBAL slot, as roman_session_submaps[_list]_dev wrote them (src local to the robot)
 *   seg_times  float64[..][2], frame_times float64[..], frame_pos float64[..][3] (thin), frame_desc float64[..][d] (want_mean): the
 *              session's tables, robot r's rows at seg0 / frame0
 *   L, list    int32[L] global slots, strictly ascending, each inside a robot's [sub0, sub0 + n_sub)
 * Per LISTED slot g of robot r the rule is roman_frame_select_dev's, over that robot's segment rows and its Nf_r frames [REF
 * roman/map/map.py:210-242]: span, candidates (lo <= t <= hi), thinning in ascending index with sqrt((dx^2 + dy^2) + dz^2) and no
 * fused multiply-adds, the mean in ascending frame index — the same per-submap code, bit for bit.
 *   mask       uint64: row of slot g at mask_off_r + (g - sub0_r) * mask_words_r; ALL mask_words_r words of a listed row are written,
 *              zero beyond the frames
 *   n_sel      int32[S], span float64[S][2], mean float64[S][d] (want_mean), by global slot
 *   changed    int32[L]: 1 when a mask word, n_sel or (want_mean) 64 bits of a mean column — NaN by its bits — of slot list[l]
 *              differs from what the slot held when the call began, else 0; always written
 * UNLISTED slots: not one byte is written.  L == 0, R == 0 and Nf_r == 0 are legal.
 * Errors, in this order, judged on host memory before the context: what roman_frame_select_dev refuses of fparams, cap and d
 * (fparams NULL, d < 0, cap < 1, reserved words, thin_dist, want_mean with d < 1); R < 0, robots NULL with R > 0; per robot a
 * reserved word not 0, a negative size or offset, mask_words_r < ceil(Nf_r / 64), ranges not ascending and disjoint; L < 0, list NULL
 * with L > 0, an entry outside every robot's slots, a list not strictly ascending -> ROMAN_E_INVALID; slots * cap beyond the index
 * width -> ROMAN_E_TOO_LARGE; then (L > 0) a NULL pointer that is needed -> ROMAN_E_INVALID; then the context.
 */
ROMAN_API int roman_session_frame_select_list_dev(roman_ctx_t* ctx, const roman_frame_select_params_t* fparams, int32_t R,
                                                  const roman_session_frame_robot_t* robots, int32_t cap,
                                                  const int32_t* count, const int32_t* src, const double* seg_times,
                                                  const double* frame_times, const double* frame_pos, int32_t d, const double* frame_desc,
                                                  int32_t L, const int32_t* list,
                                                  uint64_t* mask, int32_t* n_sel, double* span, double* mean, int32_t* changed);

/* The same with HOST pointers everywhere.  Synchronous: the tables go up over the extent the robots' ranges span, the caller's CURRENT
   mask, n_sel, span and mean go up too (`changed` compares with them, and an unlisted slot comes back as it was),
   roman_session_frame_select_list_dev runs, and mask, n_sel, span, mean and changed come back. */
ROMAN_API int roman_session_frame_select_list(roman_ctx_t* ctx, const roman_frame_select_params_t* fparams, int32_t R,
                                              const roman_session_frame_robot_t* robots, int32_t cap,
                                              const int32_t* count, const int32_t* src, const double* seg_times,
                                              const double* frame_times, const double* frame_pos, int32_t d, const double* frame_desc,
                                              int32_t L, const int32_t* list,
                                              uint64_t* mask, int32_t* n_sel, double* span, double* mean, int32_t* changed);

/*
 * roman_stacked_sim_dev: Submap.similarity for 2-D (stacked) descriptors [REF roman/map/map.py:155-162] for every pair of an
 * S0 x S1 grid, from the two maps' frame tables and the masks roman_frame_select_dev wrote.  Every pointer DEVICE; a PURE ENQUEUE
 * on the context's stream.
 *   desc_r     float64[Nf_r][d]: the frame descriptors of map r;  mask_r  uint64[S_r][ceil(Nf_r / 64)]
 *   sim[i * S1 + j] = max over a in mask0[i], b in mask1[j] of c(a, b);   c(a, b) = 0 when |a| |b| <= 1e-9, dot(a, b) / (|a| |b|) otherwise
 * Every DISTINCT frame pair is contracted once (f64 matrix core), whatever number of submaps hold it; the norms are computed once
 * per frame.  The maximum is taken in two exact stages (R[i][b] = max over a in mask0[i] of c(a, b), then the maximum over
 * b in mask1[j]), without floating-point atomics.  max of finite doubles is exact and order-free; the only rounding is inside c,
 * whose d-long sums have a fixed order: two calls agree bit for bit, whatever the band height.  The frame-cosine matrix goes in row
 * BANDS of map 0's frames through a workspace the context owns (roman_ctx_set_stacked_band), sized once per call; a failed
 * allocation returns ROMAN_E_NOMEM, nothing is enqueued and the context stays usable.
 * An empty mask on either side gives -inf (the maximum over nothing).  Descriptors must be finite: the effect of a NaN is
 * unspecified.  S0 == 0, S1 == 0 or an Nf of 0 are legal: nothing is written, or -inf where a pair exists.
 * Errors: d < 1, negative sizes, a NULL pointer that is needed -> ROMAN_E_INVALID; S0 * S1 beyond int32 -> ROMAN_E_TOO_LARGE.
 */
ROMAN_API int roman_stacked_sim_dev(roman_ctx_t* ctx, int32_t d, int32_t Nf0, const double* desc0, int32_t S0, const uint64_t* mask0,
                                    int32_t Nf1, const double* desc1, int32_t S1, const uint64_t* mask1, double* sim);

/* The same with HOST pointers everywhere.  Synchronous. */
ROMAN_API int roman_stacked_sim(roman_ctx_t* ctx, int32_t d, int32_t Nf0, const double* desc0, int32_t S0, const uint64_t* mask0,
                                int32_t Nf1, const double* desc1, int32_t S1, const uint64_t* mask1, double* sim);

/* Rows of map 0's frames one band of roman_stacked_sim* takes: 0 (the default) sizes the band workspace to at most 64 MiB; any
   other value is rounded up to a multiple of 32, the smallest band.  The result does not depend on it. */
ROMAN_API int roman_ctx_set_stacked_band(roman_ctx_t* ctx, int32_t rows);

/* ------------------------------------------------------------------------------------------- */
/* pass 1 of the pair loop over a whole grid of submaps (radius mode)                          */
/* ------------------------------------------------------------------------------------------- */

/* What the reference decides about a pair of submaps before it registers them ([REF roman/align/submap_align.py:93-149]), for
   every pair (i, j) of an S0 x S1 grid at once, on the device: the distance between the centres and the radius gate, the
   reference transform T_ij and its yaw, the cosine of the two submap descriptors [REF roman/map/map.py:144-153], skip_distance
   [REF :136] and the descriptor threshold [REF :144-149] — and the pairs that go on to register(), compacted in the order of
   the reference's loop with what the loop-closure tail needs for each (roman_lc_tail_dev's T_ref and enable).  Radius mode,
   vector (1-D) descriptors — mean_semantic, or the means roman_frame_select_dev wrote — or none; stacked frame descriptors go
   through roman_stacked_sim_dev and roman_grid_gate_sim_dev below.  The AABB mode (force_fill_submaps / no radius) is
   roman_grid_gate_aabb_dev further down; the shared-segment removal of single_robot_lc is roman_shared_reduce_dev
   (§4.11).  DESIGN.md §4.9 is the contract.  Bits of flags[]: */
#define ROMAN_GRID_NEARBY  1   /* dist < 2 * radius (strict) — the AABB gate: the boxes intersect —: robots_nearby_mat holds dist, submap_yaw_diff_mat the yaw [REF :101-103, :127-129] */
#define ROMAN_GRID_SKIP    2   /* dist > skip_distance [REF :136]: no registration, association count 0                                    */
#define ROMAN_GRID_GATED   4   /* not skipped and sim < desc_thresh [REF :144-149]: the sentinels of [REF :179-184]                         */
#define ROMAN_GRID_TODO    8   /* neither: the pair is registered; it is in the compact list                                               */

typedef struct roman_grid_gate_params {
    double  radius;            /* SubmapAlignParams.submap_radius; NaN: ROMAN_E_INVALID; < 0 ("no radius"): ROMAN_E_UNSUPPORTED (the AABB gate does not read it) */
    double  skip_distance;     /* SubmapAlignInputOutput.skip_distance; +inf is legal (nothing is skipped)                                  */
    int32_t desc_dim;          /* d: length of a submap descriptor; 0: no descriptor (sim = +inf)                                          */
    int32_t reserved0;         /* must be 0                                                                                                */
    double  desc_thresh;       /* SubmapAlignParams.submap_descriptor_thresh                                                               */
    int32_t single_robot_lc;   /* 0/1: evaluate the time gate of [REF roman/align/results.py:160-162] into enable[]                        */
    int32_t reserved1;         /* must be 0                                                                                                */
    double  lc_time_thresh;    /* SubmapAlignParams.single_robot_lc_time_thresh                                                            */
    int32_t reserved[2];       /* must be 0                                                                                                */
} roman_grid_gate_params_t;

/*
 * roman_grid_gate_dev [REF roman/align/submap_align.py:93-149]: every pointer DEVICE; a PURE ENQUEUE on the context's stream,
 * complete once that stream is synchronised.  Per side r (0: rows i, 1: columns j) arrays over that side's S_r submaps:
 *   pos_r      float64[S_r][3]   submap.position
 *   pos_gt_r   float64[S_r][3] or NULL: submap.position_gt.  The distance is taken on pos_gt when BOTH sides give it, on pos
 *              otherwise [REF :96-99]
 *   T_w_r      float64[S_r][16] row-major 4x4: the gravity-aligned pose the reference transform is built from (ground truth or
 *              not [REF :118-126]: the caller resolves that)
 *   time_r     float64[S_r]      submap.time (read only with single_robot_lc)
 *   desc_r     float64[S_r][desc_dim], or NULL when desc_dim == 0
 * Per pair, p = i * S1 + j:
 *   dist       sqrt((dx^2 + dy^2) + dz^2), without fused multiply-adds
 *   T_ij       inv(T_w0[i]) T_w1[j] (the inverse through the cofactors of the 3x3 block, as in the tail)
 *   yaw_deg    |atan2(T_ij[1][0], T_ij[0][0]) * (180 / pi)| for a NEARBY pair, NaN otherwise [REF :127-129]
 *   sim        +inf without descriptors; otherwise dot / (|a| |b|), and 0 when |a| |b| <= 1e-9 [REF roman/map/map.py:151-153].
 *              The norms are computed once per submap; every sum over d has a fixed order: two calls agree bit for bit
 *   flags      ROMAN_GRID_*: SKIP = dist > skip_distance; GATED = !SKIP && sim < desc_thresh; TODO = !SKIP && !GATED
 * Dense outputs (S0 * S1 entries each, row-major): dist, flags (int32), yaw_deg, sim, T_ij (16 doubles per pair).
 * Compact outputs, capacity S0 * S1 slots, of which the first n_todo[0] are written and the others left untouched: the TODO
 * pairs in row-major order — the order of the reference's loop, found by a prefix sum, never by atomics:
 *   pairs      int32[.][2]   (i, j)
 *   T_ref      float64[.][16] T_ij of the pair
 *   enable     int32[.]      0 when single_robot_lc and |time0[i] - time1[j]| < lc_time_thresh, 1 otherwise
 *   n_todo     int32[1]
 * S0 == 0 or S1 == 0: ROMAN_OK, n_todo = 0, nothing else written.  Errors: a NULL pointer that is needed, S < 0, a NaN radius,
 * desc_dim < 0, desc NULL with desc_dim > 0, reserved words not 0 -> ROMAN_E_INVALID; radius < 0 -> ROMAN_E_UNSUPPORTED;
 * S0 * S1 * 16 beyond int32 -> ROMAN_E_TOO_LARGE.
 */
ROMAN_API int roman_grid_gate_dev(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                                  const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                                  const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                                  double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                  int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo);

/* The same with HOST pointers everywhere ([REF roman/align/submap_align.py:93-149] for a caller that holds NumPy arrays).
   Synchronous: copies in, runs roman_grid_gate_dev, brings every output back.  The caller's pairs, T_ref and enable go up
   first: the slots beyond n_todo come back as they were. */
ROMAN_API int roman_grid_gate(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                              const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                              const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                              double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                              int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo);

/*
 * roman_grid_gate_sim_dev: roman_grid_gate_dev on a similarity that is already there (roman_stacked_sim_dev's).  The arguments are
 * roman_grid_gate_dev's without desc0 / desc1;  sim float64[S0*S1] is an INPUT: read, never written.  gparams->desc_dim must be 0
 * (ROMAN_E_INVALID otherwise).  Everything else is roman_grid_gate_dev's contract: the flags, GATED = !SKIP && sim < desc_thresh,
 * the compact list of the TODO pairs in row-major order by a prefix sum, T_ref, enable, the untouched slots, the errors.
 */
ROMAN_API int roman_grid_gate_sim_dev(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                                      const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0,
                                      const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1,
                                      double* dist, int32_t* flags, double* yaw_deg, const double* sim, double* T_ij,
                                      int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo);

/* The same with HOST pointers everywhere.  Synchronous; sim goes up and is not brought back. */
ROMAN_API int roman_grid_gate_sim(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                                  const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0,
                                  const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1,
                                  double* dist, int32_t* flags, double* yaw_deg, const double* sim, double* T_ij,
                                  int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo);

/* ------------------------------------------------------------------------------------------- */
/* force-fill submaps, the boxes of a pool and the bounding-box gate                           */
/* ------------------------------------------------------------------------------------------- */

/* The other way of cutting a map into submaps (force_fill_submaps [REF roman/map/map.py:264-295]: overlapping slices of max_size
   segments of the time-sorted map) and the other "robots nearby" gate (aabb_intersects over segments_as_global_points,
   [REF roman/align/submap_align.py:101-103], [REF roman/utils.py:160-169], [REF roman/map/map.py:133-139]: force_fill_submaps or
   no submap_radius).  DESIGN.md §4.12 is the contract. */

/*
 * roman_submaps_fill_dev: the gather half of roman_submaps_dev over lists the caller made (the ordering of [REF :267-271] is
 * sequential and small: roman_amd.align.submaps.fill_centers).  Bulk pointers DEVICE, the descriptors HOST (the library stages
 * them; pos, time, t_lo and t_hi are not read).  A PURE ENQUEUE on the context's stream.  No membership test, no sort.
 *   seg_feats  float64[N][F], seg_ids int64[N] or NULL: the map table, as for roman_submaps_dev
 *   count      int32[S]: rows of each submap, 0 <= count[s] <= cap;  src int32[S*cap]: rows [s*cap, s*cap + count[s]) are map
 *              indices in [0, N).  The device call trusts both; the host call checks them (ROMAN_E_INVALID)
 *   pool       float64[S*cap][point_dim + F - 3]: row r of submap s is segment src[s*cap + r], its centre through T_center_odom with
 *              roman_submaps_dev's arithmetic (((r0 x + r1 y) + r2 z) + t, no fused multiply-adds), every other column bit for bit;
 *              rows beyond count[s] are not written
 *   ids_out    int64[S*cap] or NULL (needs seg_ids)
 *   desc_dim, desc_out   float64[S][desc_dim] or NULL: 'mean_semantic' in output order, as roman_submaps_dev writes it
 * S == 0 and N == 0 are legal.  Errors: bad dims (point_dim, F < 3, N / S < 0, desc_dim outside [0, F - 3]), cap < 1, a NULL
 * pointer that is needed -> ROMAN_E_INVALID.
 */
ROMAN_API int roman_submaps_fill_dev(roman_ctx_t* ctx, int32_t point_dim, int32_t cap, int32_t N, int32_t F,
                                     const double* seg_feats, const int64_t* seg_ids, int32_t S, const roman_submap_desc_t* descs,
                                     const int32_t* count, const int32_t* src, double* pool, int64_t* ids_out,
                                     int32_t desc_dim, double* desc_out);

/* The same with HOST pointers everywhere.  Synchronous; pool may be NULL (only ids_out / desc_out come back).  The caller's pool,
   ids_out and desc_out go up first: what the device call leaves untouched comes back as it was. */
ROMAN_API int roman_submaps_fill(roman_ctx_t* ctx, int32_t point_dim, int32_t cap, int32_t N, int32_t F,
                                 const double* seg_feats, const int64_t* seg_ids, int32_t S, const roman_submap_desc_t* descs,
                                 const int32_t* count, const int32_t* src, double* pool, int64_t* ids_out,
                                 int32_t desc_dim, double* desc_out);

/*
 * roman_submap_boxes_dev: what aabb_intersects reads of Submap.segments_as_global_points [REF roman/map/map.py:133-139] for the
 * S submaps of a pool.  Every pointer DEVICE; a PURE ENQUEUE on the context's stream.
 *   pool       float64[S*cap][F], F >= 3: the first three columns of rows [s*cap, s*cap + count[s]) are read (a pool built
 *              with point_dim 2 holds no z and cannot be used)
 *   count      int32[S]
 *   T_odom_center  float64[S][16] row-major 4x4: the pose that takes submap s to the global frame (the caller resolves
 *              ground truth or not, as has_gt does [REF :138])
 *   box        float64[S][6] = (min x, min y, min z, max x, max y, max z) of the rows' points in the global frame, each component
 *              ((r0 x + r1 y) + r2 z) + t, without fused multiply-adds.  min / max of finite doubles are exact and order-free: two
 *              calls agree bit for bit.  count[s] == 0: (+inf, +inf, +inf, -inf, -inf, -inf) — never nearby.
 * Inputs must be finite.  S == 0 is legal.  Errors: S < 0, F < 3, cap < 1, a NULL pointer that is needed -> ROMAN_E_INVALID.
 */
ROMAN_API int roman_submap_boxes_dev(roman_ctx_t* ctx, int32_t S, int32_t F, int32_t cap, const double* pool, const int32_t* count,
                                     const double* T_odom_center, double* box);

/* The same with HOST pointers everywhere.  Synchronous. */
ROMAN_API int roman_submap_boxes(roman_ctx_t* ctx, int32_t S, int32_t F, int32_t cap, const double* pool, const int32_t* count,
                                 const double* T_odom_center, double* box);

/*
 * roman_grid_gate_aabb_dev: roman_grid_gate_dev with the bounding-box gate [REF roman/align/submap_align.py:101-103].  The first
 * 23 arguments are roman_grid_gate_dev's; then
 *   box0 float64[S0][6], box1 float64[S1][6]: as roman_submap_boxes_dev wrote them.  NEARBY(i, j) is the six comparisons of
 *              [REF roman/utils.py:167-169]: min0 <= max1 and max0 >= min1 on every axis — <= and >= as they stand: touching boxes
 *              intersect; an empty submap's box intersects nothing.  gparams->radius is NOT read (any value, NaN included)
 *   sim_in     float64[S0*S1] or NULL.  Given: the similarity of every pair is already there (roman_stacked_sim_dev's), read as
 *              roman_grid_gate_sim_dev reads it and never written; gparams->desc_dim must then be 0 (ROMAN_E_INVALID otherwise),
 *              desc0 / desc1 are not read and `sim` is not written (it may be NULL)
 * Everything else is roman_grid_gate_dev's contract, untouched: dist, T_ij, yaw_deg for NEARBY pairs only, sim, SKIP / GATED / TODO,
 * the compact list of the TODO pairs in row-major order by a prefix sum (no atomics), T_ref, enable, the untouched slots, the
 * errors — without those of the radius, plus box NULL -> ROMAN_E_INVALID.  Every pointer DEVICE; a PURE ENQUEUE on the context's stream.
 */
ROMAN_API int roman_grid_gate_aabb_dev(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                                       const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                                       const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                                       double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                       int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo,
                                       const double* box0, const double* box1, const double* sim_in);

/* The same with HOST pointers everywhere.  Synchronous: copies in, runs roman_grid_gate_aabb_dev, brings every output back (sim
   only without sim_in).  The caller's pairs, T_ref and enable go up first: the slots beyond n_todo come back as they were. */
ROMAN_API int roman_grid_gate_aabb(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t S0, int32_t S1,
                                   const double* pos0, const double* pos_gt0, const double* T_w0, const double* time0, const double* desc0,
                                   const double* pos1, const double* pos_gt1, const double* T_w1, const double* time1, const double* desc1,
                                   double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                   int32_t* pairs, double* T_ref, int32_t* enable, int32_t* n_todo,
                                   const double* box0, const double* box1, const double* sim_in);

/*
 * roman_session_gate_dev: pass 1 [REF roman/align/submap_align.py:93-149] of EVERY robot pair of a multi-robot
 * session — the loop of [REF demo/demo.py:138-161] — in one launch sequence: roman_grid_gate_dev over a list of grids ("blocks") that
 * share one set of per-submap arrays.  Every bulk pointer DEVICE; a PURE ENQUEUE on the context's stream.  The small tables travel
 * twice: on the device (the kernels read them) and as `_host` copies (the library validates them without a read-back).
 *
 *   R, sub_off int32[R+1]   robot r owns the global submaps [sub_off[r], sub_off[r+1]); sub_off[0] = 0, S = sub_off[R]
 *   pos        float64[S*3]; pos_gt float64[S*3] or NULL; has_gt int32[R], read only with pos_gt: a block's distance is between the
 *              ground-truth centres when BOTH its robots have has_gt set, between pos otherwise [REF :96-99]
 *   T_w        float64[S*16]; time float64[S] (may be NULL when no block sets self_lc); desc float64[S*desc_dim] or NULL (desc_dim 0)
 *   nb, blocks int32[nb*4]: (r0, r1, self_lc, reserved = 0): the grid of r0's submaps (rows) against r1's (columns); self_lc is the
 *              block's single_robot_lc: the time gate into `enable`.  gparams->single_robot_lc is NOT read; every other field of
 *              gparams holds for all blocks.  A robot pair (r0, r1) may be listed once.
 *   pair_off   int64[nb+1]: prefix of n0 * n1;  tile_off int64[nb+1]: prefix of n0 * ceil(n1 / 4) — from sub_off and blocks
 *
 * Dense outputs (pair_off[nb] entries; block b row-major at pair_off[b]): dist, flags, yaw_deg, sim, T_ij (x16) — per block bit for
 * bit what roman_grid_gate_dev writes for its two sides.  Compact outputs (capacity pair_off[nb]; slots beyond the total untouched):
 *   pairs      int32[.][2] GLOBAL submap indices (gi, gj) of the TODO pairs: blocks in list order, row-major within a block
 *   T_ref, enable   roman_grid_gate_dev's contract; enable = 0 only where the block's self_lc is set and |time[gi] - time[gj]| < lc_time_thresh
 *   todo_off   int32[nb+1]: block b's TODO pairs are the slots [todo_off[b], todo_off[b+1]); todo_off[nb] is the total
 * No atomics: two runs agree bit for bit.
 *
 * nb == 0 or no pair at all (robots without submaps): ROMAN_OK, todo_off all 0, nothing else written.  Errors: a NULL pointer that
 * is needed, R < 0, nb < 0, r outside [0, R), sub_off decreasing or not starting at 0, a reserved word not 0, a NaN radius,
 * desc_dim < 0, a robot pair listed twice, pair_off / tile_off that disagree with sub_off and blocks -> ROMAN_E_INVALID;
 * radius < 0 -> ROMAN_E_UNSUPPORTED (the gate without a radius is roman_session_gate_aabb_dev below); pair_off[nb] * 16 beyond int32
 * -> ROMAN_E_TOO_LARGE.
 */
ROMAN_API int roman_session_gate_dev(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                                     const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                     int32_t nb, const int32_t* blocks, const int32_t* blocks_host,
                                     const int64_t* pair_off, const int64_t* pair_off_host, const int64_t* tile_off, const int64_t* tile_off_host,
                                     double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                     int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off);

/* The same with HOST pointers everywhere (each table once).  Synchronous: copies in, runs roman_session_gate_dev, brings every
   output back with one synchronisation.  The caller's pairs, T_ref and enable go up first: the slots beyond todo_off[nb] come back
   as they were. */
ROMAN_API int roman_session_gate(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                                 const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                 int32_t nb, const int32_t* blocks, const int64_t* pair_off, const int64_t* tile_off,
                                 double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                 int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off);

/*
 * roman_session_gate_sim_dev: roman_session_gate_dev over a similarity that is ALREADY computed — what
 * roman_grid_gate_sim_dev is to roman_grid_gate_dev.  The arguments are roman_session_gate_dev's plus a trailing
 *   sim_in     float64[pair_off[nb]], DEVICE: block b's similarities row-major at pair_off[b] (roman_session_stacked_sim_dev writes them so)
 * gparams->desc_dim must be 0 (else ROMAN_E_INVALID): desc_thresh gates sim_in, GATED = not skipped and sim_in < desc_thresh, so a
 * similarity equal to the threshold passes and -inf is gated.  `desc` is not read and `sim` is not written; both may be NULL.
 * Every other output, per block, is bit for bit what roman_grid_gate_sim_dev writes when given that block's slice of sim_in.
 * Errors: roman_session_gate_dev's, and sim_in NULL while a pair exists -> ROMAN_E_INVALID.
 */
ROMAN_API int roman_session_gate_sim_dev(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                                         const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                         int32_t nb, const int32_t* blocks, const int32_t* blocks_host,
                                         const int64_t* pair_off, const int64_t* pair_off_host, const int64_t* tile_off, const int64_t* tile_off_host,
                                         double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                         int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* sim_in);

/* The same with HOST pointers everywhere (each table once).  Synchronous; sim_in goes up and is not brought back. */
ROMAN_API int roman_session_gate_sim(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                                     const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                     int32_t nb, const int32_t* blocks, const int64_t* pair_off, const int64_t* tile_off,
                                     double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                     int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* sim_in);

/*
 * roman_session_stacked_sim_dev: roman_stacked_sim_dev for EVERY block of a session in one launch sequence, over
 * ONE frame table.  Every bulk pointer DEVICE; a PURE ENQUEUE on the context's stream.  The small tables travel twice, as
 * roman_session_gate_dev's do: on the device (the kernels read them) and as `_host` copies (validated without a read-back, in front
 * of everything else: every refusal has its code even without a device).
 *
 *   d, Nf, desc        float64[Nf][d]: the frame descriptors of the whole session
 *   mask               uint64 words: the frame masks of all views (roman_frame_select_dev's rows, gathered)
 *   R, per view r      frame_lo[r], frame_n[r] (int32): the view's frames are the rows [frame_lo[r], frame_lo[r] + frame_n[r]) of desc;
 *                      mask_off[r] (int64, in words): its masks are uint64[n_r][ceil(frame_n[r] / 64)] at mask + mask_off[r], bit t of a
 *                      row = frame frame_lo[r] + t; n_r = sub_off[r+1] - sub_off[r].  These are ranges, not prefixes: two views of one
 *                      robot may name the same frames and the same words — everything is read-only
 *   sub_off, nb, blocks, pair_off   roman_session_gate_dev's tables; self_lc and the reserved word are validated as there, self_lc
 *                      is not otherwise read
 *   sim                float64[pair_off[nb]]: block b row-major at pair_off[b].  Slots outside [0, pair_off[nb]) are untouched
 *
 * Per block, sim is BIT FOR BIT what roman_stacked_sim_dev writes for the block's two sides: -inf for an empty mask or a view without
 * frames, 0 where |a| |b| <= 1e-9.  The norms are computed once per frame of the session.  No floating-point atomics; two runs agree
 * bit for bit; the result does not depend on roman_ctx_set_stacked_band or on the other blocks of the list.  The frame-cosine
 * matrices go through the context's band workspace in ROUNDS of at most one row band per block, a round's bands together within
 * 64 MiB (one band of 32 rows may exceed it; a band height set with roman_ctx_set_stacked_band caps every band).
 * nb == 0 or no pair at all: ROMAN_OK, nothing written.  A failed workspace allocation: ROMAN_E_NOMEM, nothing enqueued, the
 * context stays usable.
 * Errors (ROMAN_E_INVALID): d < 1, Nf < 0, R < 0, nb < 0, a frame range outside [0, Nf], a negative mask_off, a NULL pointer that is
 * needed, and everything roman_session_gate_dev refuses about sub_off, blocks and pair_off.
 * ROMAN_E_TOO_LARGE, over the blocks with submaps and frames on both sides (n0 x n1 submaps, Nf0 x Nf1 frames):
 *   pair_off[nb] * 16 beyond int32 (roman_session_gate_dev's bound);
 *   sum of n0 * ceil(Nf1 / 256) beyond int32 (the workgroups of one round's column maxima);
 *   sum of ceil(Nf0 / 32) * ceil(Nf1 / 32) beyond int32 (the tiles of one round, and the number of bands).
 * Offsets into the frame table, the masks and the workspaces are 64-bit.
 */
ROMAN_API int roman_session_stacked_sim_dev(roman_ctx_t* ctx, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask,
                                            int32_t R, const int32_t* frame_lo, const int32_t* frame_lo_host, const int32_t* frame_n, const int32_t* frame_n_host,
                                            const int64_t* mask_off, const int64_t* mask_off_host, const int32_t* sub_off, const int32_t* sub_off_host,
                                            int32_t nb, const int32_t* blocks, const int32_t* blocks_host, const int64_t* pair_off, const int64_t* pair_off_host,
                                            double* sim);

/* The same with HOST pointers everywhere (each table once).  Synchronous.  mask_words: the words `mask` holds (the call copies them):
   a view whose masks leave them -> ROMAN_E_INVALID. */
ROMAN_API int roman_session_stacked_sim(roman_ctx_t* ctx, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask, int64_t mask_words,
                                        int32_t R, const int32_t* frame_lo, const int32_t* frame_n, const int64_t* mask_off, const int32_t* sub_off,
                                        int32_t nb, const int32_t* blocks, const int64_t* pair_off, double* sim);

/*
 * roman_session_stacked_sim_list_dev: roman_session_stacked_sim_dev for an explicit LIST of pairs — what a session
 * that grows asks for: the similarity of the pairs a new or changed submap touches, not of whole blocks.  The arguments up to
 * pair_off_host are roman_session_stacked_sim_dev's.  Every bulk pointer DEVICE; a PURE ENQUEUE on the context's stream (the norms of
 * the frame table, then one wave per listed pair); the small tables and the list travel twice (device, and `_host` copies).
 *
 *   L, list    int32[L][3]: (b, i, j) — roman_session_gate_list_dev's list, strictly ascending, validated by the same code
 *   sim        float64[pair_off[nb]] in the DENSE layout: for each listed pair the call writes sim[pair_off[b] + i * n1 + j], BIT FOR
 *              BIT what roman_session_stacked_sim_dev writes there over the same tables (-inf for an empty mask or a view without
 *              frames, 0 where |a| |b| <= 1e-9).  No other element of sim is read or written:
 *              roman_session_gate_list_dev(..., sim_in = sim) follows on the same stream
 *
 * No atomics, no band workspace; two runs agree bit for bit; a pair's result does not depend on which other pairs are listed.  A
 * mask may select any number of frames.  L == 0: ROMAN_OK, nothing written.  A failed allocation of the norms: ROMAN_E_NOMEM,
 * nothing enqueued, the context stays usable.
 * Errors, judged on host memory in front of everything else (a NULL context included), in this order: what
 * roman_session_gate_dev refuses about sub_off, blocks and pair_off; d < 1, a frame range outside [0, Nf], a negative mask_off, a
 * NULL desc / mask that is needed; then L < 0, a NULL list with L > 0, an entry with b outside [0, nb) or (i, j) outside its
 * block, a list not strictly ascending, a NULL sim with L > 0 -> ROMAN_E_INVALID.  The `_host` copies are judged in front of the
 * device pointers: a NULL device table or device list is refused (ROMAN_E_INVALID) behind all of the above.
 * desc and mask are needed — and read — only while a block has submaps and frames on BOTH sides.  Without such a block both may
 * be NULL whatever Nf and L are: every listed pair is -inf, the norms are not computed and neither pointer is touched.
 */
ROMAN_API int roman_session_stacked_sim_list_dev(roman_ctx_t* ctx, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask,
                                                 int32_t R, const int32_t* frame_lo, const int32_t* frame_lo_host, const int32_t* frame_n, const int32_t* frame_n_host,
                                                 const int64_t* mask_off, const int64_t* mask_off_host, const int32_t* sub_off, const int32_t* sub_off_host,
                                                 int32_t nb, const int32_t* blocks, const int32_t* blocks_host, const int64_t* pair_off, const int64_t* pair_off_host,
                                                 int32_t L, const int32_t* list, const int32_t* list_host, double* sim);

/* The same with HOST pointers everywhere (each table and the list once).  Synchronous.  The caller's sim goes up first: the entries
   that are not listed come back as they were.  mask_words as roman_session_stacked_sim takes it. */
ROMAN_API int roman_session_stacked_sim_list(roman_ctx_t* ctx, int32_t d, int32_t Nf, const double* desc, const uint64_t* mask, int64_t mask_words,
                                             int32_t R, const int32_t* frame_lo, const int32_t* frame_n, const int64_t* mask_off, const int32_t* sub_off,
                                             int32_t nb, const int32_t* blocks, const int64_t* pair_off, int32_t L, const int32_t* list, double* sim);

/*
 * roman_session_boxes_dev: roman_submap_boxes_dev — what aabb_intersects [REF roman/utils.py:160-169] reads of
 * Submap.segments_as_global_points [REF roman/map/map.py:133-139] — over the submap table of a whole session instead of one pool's
 * slots.  Every pointer DEVICE; a PURE ENQUEUE on the context's stream; one launch, no launch per robot, no gather of rows.
 *   S          global submaps: the submaps of every VIEW of the session (§4.14), sub_off[R] of roman_session_gate_dev
 *   pool       float64[.][F], F >= 3: ONE pool, the concatenated pools the batch reads; only the first three columns are read
 *   row0       int64[S], count int32[S]: submap g holds the rows [row0[g], row0[g] + count[g]) of pool.  Ranges, not prefixes: in
 *              any order, and two views of one robot name the SAME rows with their own transform — everything but box is read-only.
 *              The device call trusts both; the host call refuses a negative entry (ROMAN_E_INVALID) and copies the rows they name
 *   T_odom_center  float64[S][16] row-major 4x4: the pose that takes submap g to the global frame (ground truth or not, as has_gt
 *              does [REF roman/map/map.py:138]: the caller resolves that)
 *   box        float64[S][6] = (min x, min y, min z, max x, max y, max z), each component ((r0 x + r1 y) + r2 z) + t without fused
 *              multiply-adds: for any submap BIT FOR BIT what roman_submap_boxes_dev writes for the same rows and the same
 *              transform.  count[g] == 0: (+inf, +inf, +inf, -inf, -inf, -inf).  No atomics: two calls agree bit for bit
 * Inputs must be finite.  S == 0: ROMAN_OK, nothing written.  Errors: S < 0, F < 3, a NULL pointer that is needed -> ROMAN_E_INVALID.
 */
ROMAN_API int roman_session_boxes_dev(roman_ctx_t* ctx, int32_t S, int32_t F, const double* pool, const int64_t* row0, const int32_t* count,
                                      const double* T_odom_center, double* box);

/* The same with HOST pointers everywhere.  Synchronous; `pool` is read up to the last row a submap names. */
ROMAN_API int roman_session_boxes(roman_ctx_t* ctx, int32_t S, int32_t F, const double* pool, const int64_t* row0, const int32_t* count,
                                  const double* T_odom_center, double* box);

/*
 * roman_segment_shapes_dev: the segment table of a map from the segments' POINT CLOUDS — what the reference computes
 * per segment in a Python loop before anything else: submaps_from_roman_map calls set_center_ref on every segment and then
 * roman_map.minimal_data() [REF roman/map/map.py:258-262], which reads center, volume, linearity, planarity, scattering and extent of
 * every Segment [REF roman/object/segment.py:496-508].  Bulk data on the DEVICE; a PURE ENQUEUE on the context's stream.
 *   points        float64[P][3], odom frame: the clouds of all segments one behind the other, P = seg_off_host[N]
 *   seg_off_dev   int64[N + 1] on the device, seg_off_host the same numbers on the HOST (the launch is sized from them; reading the
 *                 device copy would cost a synchronisation): ascending, [0] == 0; segment i owns the rows [seg_off[i], seg_off[i + 1])
 *   params        roman_segment_shape_params_t below
 *   out           float64[N][out_stride]: row i receives, at the columns the block names and NOWHERE else,
 *                   col_center + 0..2   the centre.  ROMAN_CENTER_MEAN: the mean [REF roman/object/segment.py:271-272].
 *                                       ROMAN_CENTER_BOTTOM_MIDDLE: np.median of x and of y — for an even count (a + b) * 0.5 of the two
 *                                       middle order statistics — and the minimum of z [REF :267-270]: a selection, EXACT (a median that is a zero
 *                                       is +0.0, as np.median's mean step gives it; the minimum orders -0.0 below +0.0)
 *                   col_pca + 0..2      linearity (e0 - e1) / e0, planarity (e1 - e2) / e0, scattering e2 / e0 [REF :445-472] of the
 *                                       eigenvalues e0 >= e1 >= e2 (absolute values: the singular values of [REF :441]) of the 3 x 3
 *                                       population covariance, taken about the mean in the CENTRED form sum (x - m)(x - m)' / n.
 *                                       (open3d's compute_mean_and_covariance [REF :430] uses E[xx'] - mm', which cancels digits away
 *                                       far from the origin: DESIGN.md §2.)  A zero covariance gives 0 / 0 = NaN, nothing is clamped
 *                   col_extent + 0..2   the side lengths of the box of the points in the eigenframe of that covariance, ASCENDING
 *                                       (every consumer reads sorted(extent)); col_volume their product [REF :244-263].  n <= 4: 0
 *                                       [REF :253, :260].  UNPINNED against open3d's create_from_points
 *   status        int32[N]: ROMAN_SEG_* flags below
 * Sums run in a fixed order (no floating-point atomics): two calls give the same bits, and a segment's row depends on its own
 * points only — not on its place in the list.  A segment of fewer than ROMAN_SEG_BLOCK_MIN points is one wave's, the others take a
 * workgroup each; the two paths agree within the rounding bound of DESIGN.md §4.24, each is deterministic on its own.
 * The contents of device arrays are not validated: seg_off_dev must hold what seg_off_host holds; non-finite points give
 * unspecified values for their own segment and for no other.  N == 0: ROMAN_OK, nothing enqueued.
 * Errors (ROMAN_E_INVALID, nothing enqueued): NULL ctx, params, seg_off_dev (N > 0) or seg_off_host; N < 0; seg_off_host[0] != 0 or
 * descending; an unknown center_ref; out_stride < 1; col_center < 0 or another column < -1; a written column range that leaves
 * out_stride; two written ranges that overlap; non-zero reserved words; NULL points with P > 0; NULL out / status with N > 0.
 * A segment of more than INT32_MAX points: ROMAN_E_TOO_LARGE.
 */
#define ROMAN_CENTER_MEAN           0
#define ROMAN_CENTER_BOTTOM_MIDDLE  1
#define ROMAN_SEG_EMPTY        1   /* n == 0: the named columns of the row are zeros (ROMAN_SEG_FEW_POINTS is set as well) */
#define ROMAN_SEG_FEW_POINTS   2   /* n <= 4: no box, extent and volume are 0 [REF roman/object/segment.py:253, :260]          */
#define ROMAN_SEG_DEGENERATE   4   /* e0 == 0 (one point, or all points equal): the three ratios are NaN                     */
#define ROMAN_SEG_BLOCK_MIN  768   /* points from which a segment takes a workgroup instead of a wave (roman_ctx_set_segment_block_min) */
typedef struct roman_segment_shape_params {
    int32_t center_ref;            /* ROMAN_CENTER_MEAN / ROMAN_CENTER_BOTTOM_MIDDLE */
    int32_t out_stride;            /* doubles per row of `out` */
    int32_t col_center;            /* first of 3 columns */
    int32_t col_pca;               /* first of 3 columns, or -1: not written */
    int32_t col_volume;            /* 1 column, or -1 */
    int32_t col_extent;            /* first of 3 columns, or -1 */
    int32_t reserved[2];           /* must be 0 */
} roman_segment_shape_params_t;
ROMAN_API int roman_segment_shapes_dev(roman_ctx_t* ctx, const double* points, const int64_t* seg_off_dev, const int64_t* seg_off_host, int32_t N,
                                       const roman_segment_shape_params_t* params, double* out, int32_t* status);

/* The same with HOST pointers everywhere.  Synchronous; `out` goes up first, so the columns that are not named come back as they were. */
ROMAN_API int roman_segment_shapes(roman_ctx_t* ctx, const double* points, const int64_t* seg_off, int32_t N,
                                   const roman_segment_shape_params_t* params, double* out, int32_t* status);

/* Measurement only: the point count from which roman_segment_shapes* hands a segment to a workgroup (0: ROMAN_SEG_BLOCK_MIN again).
   It changes which path a segment takes and with it the order of its sums: the rows of a context set to another value agree with
   those of the default within the bound of DESIGN.md §4.24, NOT bit for bit, and the depth D of that bound is then the one of the
   path taken.  Every documented figure and every test assumes the default. */
ROMAN_API int roman_ctx_set_segment_block_min(roman_ctx_t* ctx, int32_t n);

/*
 * roman_assoc_scores_dev: the scores of the mapper's per-frame data association — what global_nearest_neighbor
 * computes in its pair loop [REF roman/map/global_nearest_neighbor.py:23-36] for every (segment, observation) pair of a frame
 * [REF roman/map/mapper.py:65-68] and merge() again for every pair of segments [REF roman/map/mapper.py:276-299]: the voxel IoU or
 * IoM of the two point clouds, VoxelGrid.iou over VoxelGrid.from_points [REF roman/map/voxel_grid.py:32-103], optionally the cosine
 * of their descriptors [REF roman/map/mapper.py:204-212], and the score.  Bulk data on the DEVICE; a PURE ENQUEUE on the context's
 * stream: no synchronisation, no read-back.  All workspace is sized from cloud_off_host: P keys twice and one record per cloud.
 *   points          float64[P][3]: N1 + N2 clouds one behind the other (self mode: N1), P = cloud_off_host[number of clouds]
 *   cloud_off_dev   int64[clouds + 1] on the device, cloud_off_host the same numbers on the HOST: ascending, [0] == 0 (the
 *                   contract of roman_segment_shapes_dev's seg_off).  The first N1 clouds are the ROWS of the outputs, the next
 *                   N2 the COLUMNS
 *   N2              >= 0, or -1: SELF mode, the N1 clouds against themselves (N1 x N1, every ordered pair is computed)
 *   desc, d         float64[clouds][d] descriptors, read when params->semantic is 1; NULL with d == 0: no cloud has one, and the
 *                   cosine of every pair is 1.0 [REF roman/map/mapper.py:208-209]
 *   n_vox           int32[clouds] or NULL: occupied voxels of every cloud
 *   status          int32[clouds]: ROMAN_ASSOC_OK; ROMAN_ASSOC_EMPTY: no point; ROMAN_ASSOC_RANGE: a coordinate is not finite or a
 *                   voxel key needs more than 21 bits on an axis (|coordinate| / voxel_size beyond 2^20).  An EMPTY or RANGE cloud
 *                   has no voxel: n_vox 0 and geo 0.0 against everything.  (The reference's from_points raises on an empty cloud and
 *                   the mapper never passes one: this rule is this library's.)
 *   inter           int32[N1 * N2] or NULL: voxels both clouds hold inside the intersection of their integer boxes
 *   geo             float64[N1 * N2]: IoU inter / (va + vb - inter) or IoM inter / min(va, vb) of the volumes n_vox * voxel_size**3,
 *                   0.0 for a zero denominator, in the reference's operation order: bit for bit what the reference's arithmetic
 *                   gives.  One line is UNPINNED: the grid index of a point, open3d's VoxelGrid.create_from_point_cloud, is
 *                   restated by open3d's documented rule (origin = min_bound - voxel_size / 2, index = floor((p - origin) /
 *                   voxel_size)) and has not been compared with a real open3d
 *   sem             float64[N1 * N2] or NULL: the cosine; written only when params->semantic is 1.  A zero descriptor gives NaN
 *   score           float64[N1 * N2]: 1e9 where a similarity is below its range[0]; otherwise -geo (one criterion) or
 *                   -sqrt(((geo - g0) / (g1 - g0)) * ((sem - s0) / (s1 - s0))) (two; the reference writes np.power(x, 1 / 2), this
 *                   is the correctly rounded square root).  Comparisons are IEEE: a NaN similarity gives a NaN score
 * Integer counts and a fixed summation order: two calls give the same bits.  N1 == 0 or N2 == 0: ROMAN_OK, nothing written.
 * Errors (ROMAN_E_INVALID with a roman_last_error text, nothing enqueued): NULL params; voxel_size not finite or <= 0; an unknown
 * geometric method; semantic not 0 / 1; range[1] == range[0] or a NaN in a range that is in use; N1 < 0,
 * N2 < -1; NULL cloud_off_host, [0] != 0 or descending; d < 0; NULL desc with d > 0, or desc with d == 0, when semantic is 1; NULL
 * points with P > 0; NULL geo / score / status with N1, N2 != 0; NULL ctx; NULL cloud_off_dev.  More than INT32_MAX points in a
 * cloud, more than 2^30 pairs or 2^30 clouds: ROMAN_E_TOO_LARGE.
 */
#define ROMAN_ASSOC_IOU   0
#define ROMAN_ASSOC_IOM   1
#define ROMAN_ASSOC_OK    0
#define ROMAN_ASSOC_EMPTY 1
#define ROMAN_ASSOC_RANGE 2
#define ROMAN_ASSOC_WAVE_MAX  256   /* a cloud of at most so many points is sorted by one wave (roman_ctx_set_assoc_cuts)            */
#define ROMAN_ASSOC_LDS_MAX  8192   /* ... of at most so many by one workgroup in LDS; longer clouds merge through a global ping-pong */
typedef struct roman_assoc_params {
    double  voxel_size;        /* > 0, finite (iou_voxel_size) */
    int32_t geometric;         /* ROMAN_ASSOC_IOU | ROMAN_ASSOC_IOM */
    int32_t semantic;          /* 0: none, 1: cosine over `desc` */
    double  geo_range[2];      /* threshold, maximum (geometric_score_range) */
    double  sem_range[2];      /* (semantic_score_range); read when semantic is 1 */
} roman_assoc_params_t;
ROMAN_API int roman_assoc_scores_dev(roman_ctx_t* ctx, const roman_assoc_params_t* params, const double* points, const int64_t* cloud_off_dev,
                                     const int64_t* cloud_off_host, int32_t N1, int32_t N2, const double* desc, int32_t d,
                                     int32_t* n_vox, int32_t* inter, double* geo, double* sem, double* score, int32_t* status);

/* The same with HOST pointers everywhere.  Synchronous. */
ROMAN_API int roman_assoc_scores(roman_ctx_t* ctx, const roman_assoc_params_t* params, const double* points, const int64_t* cloud_off,
                                 int32_t N1, int32_t N2, const double* desc, int32_t d,
                                 int32_t* n_vox, int32_t* inter, double* geo, double* sem, double* score, int32_t* status);

/* Measurement only: the two point counts at which roman_assoc_scores* changes the kernel that sorts a cloud's keys — up to wave_max
   one wave, up to lds_max one workgroup in LDS, beyond it one workgroup that sorts chunks of lds_max keys and merges them in global
   memory.  0: the default again (ROMAN_ASSOC_WAVE_MAX, ROMAN_ASSOC_LDS_MAX); wave_max <= 512, wave_max <= lds_max, 2 <= lds_max <= 8192.
   Every path gives the same sorted keys, so results do not depend on the cuts. */
ROMAN_API int roman_ctx_set_assoc_cuts(roman_ctx_t* ctx, int32_t wave_max, int32_t lds_max);

/*
 * roman_segment_integrate_dev: the segment update of the mapper's per-frame loop — what Segment.update does to a
 * segment's cloud with every associated observation, Segment.__init__ with every new segment and update_from_segment with every
 * merge [REF roman/object/segment.py:98-161]: the added cloud, transformed into the world frame
 * [REF roman/object/segment.py:133-148], is appended to the segment's [REF roman/object/segment.py:163-175] and the whole is
 * cleaned [REF roman/object/segment.py:177-193] by open3d's voxel_down_sample(voxel_size) and, when outlier_std is in use,
 * remove_statistical_outlier(10, outlier_std).  One call takes a LIST OF JOBS.  Bulk data on the DEVICE; a PURE ENQUEUE on the
 * context's stream: no synchronisation, no read-back.
 *   points          float64[P][3]: n_clouds clouds one behind the other, P = cloud_off_host[n_clouds]
 *   cloud_off_dev   int64[n_clouds + 1] on the device, cloud_off_host the same numbers on the HOST: ascending, [0] == 0
 *   poses           float64[n_poses][16]: row-major 4 x 4 poses T_world_body [REF roman/object/segment.py:142-144]; may be NULL when no job names one
 *   jobs_dev        roman_integrate_job_t[n_jobs] on the device, jobs_host the same on the HOST.  base: the cloud of the segment,
 *                   -1 for a new segment; add: the cloud that is added; pose: the pose of the added cloud, -1 when it is in the
 *                   world frame already (a merge; the clouds of SegmentClouds.from_observations).  A cloud is the base of at
 *                   most one job
 *   SLOTS           job j owns the elements [slot_j, slot_j + n(base_j) + n(add_j)) of out_points and out_avg, slot_j the
 *                   exclusive prefix sum of n(base) + n(add) over the jobs in front of it, computed from cloud_off_host alone; all
 *                   workspace is laid out the same way, and no write of a job leaves its slot
 *   out_points      float64[total][3]: the first out_count[j] rows of slot j are job j's cleaned cloud; the rest of the slot is
 *                   left untouched.  May be NULL when total == 0 (every slot is empty)
 *   NO ALIASING     out_points, out_avg, out_count, out_status and out_thr must not overlap points, poses, cloud_off, jobs or each
 *                   other: a job copies or reads its clouds from `points` while other jobs write their slots, in no defined order.
 *                   To update clouds in place, write to a second array and swap the two between calls
 *   out_count       int32[n_jobs]: 0 is what the reference stores as points = None [REF roman/object/segment.py:188-189]
 *   out_status      int32[n_jobs], the vocabulary of roman_assoc_scores: ROMAN_ASSOC_OK; ROMAN_ASSOC_EMPTY: base and added cloud
 *                   hold no point; ROMAN_ASSOC_RANGE: a (transformed) coordinate is not finite or a voxel index needs more than 21
 *                   bits — count 0
 *   out_avg         float64[total] or NULL: with the outlier step, the mean distance of every DOWN-SAMPLED point of the job to its
 *                   min(10, m) nearest, itself included, in down-sampled order (ascending voxel key)
 *   out_thr         float64[n_jobs] or NULL: with the outlier step, the distance threshold of every job that ran it
 * Semantics (tests/_integrate_oracle.py states them line by line).  An EMPTY ADDED CLOUD returns the base unchanged, with no
 * clean-up [REF roman/object/segment.py:165-166].  Otherwise: world point ((r0 x + r1 y) + r2 z) + t per row (the rounding of the
 * reference's BLAS product is UNPINNED); base points then added points; voxel index floor((p - (min_bound - voxel_size / 2)) /
 * voxel_size) per axis — open3d's documented rule, UNPINNED: not compared with a real open3d — one output point per index, the
 * sum of its points one after another in input order from 0.0 divided by their number; output in ASCENDING VOXEL KEY (x most
 * significant; open3d's own order is that of its hash map, UNPINNED).  Then, when outlier_std is finite and > 0
 * [REF roman/params/mapper_params.py:100-103], open3d's published remove_statistical_outlier (UNPINNED in the same sense):
 * avg_i the mean of the square roots of the min(10, m) smallest squared distances (dx dx + dy dy) + dz dz, added ascending;
 * mean = sum(avg_i > 0) / m, std = sqrt(sum((avg_i - mean)^2, avg_i > 0) / (m - 1)), thr = mean + outlier_std std, both sums in
 * the fixed order of DESIGN.md §4.26; point i is kept iff avg_i > 0 && avg_i < thr.  m <= 2 gives an empty cloud.  No atomics:
 * two calls give the same bits, and so does every size class.  n_jobs == 0: ROMAN_OK, nothing written.
 * Errors (ROMAN_E_INVALID with a roman_last_error text, nothing enqueued; the argument checks run before the context is looked
 * at): NULL params; voxel_size not finite or <= 0; a NaN outlier_std; nb_neighbors != 10; a negative count; NULL cloud_off_host,
 * [0] != 0 or descending; NULL jobs_host; a job whose add, base or pose is out of range; a base cloud named by two jobs; NULL
 * poses when a job names one; NULL points with P > 0; NULL out_points / out_count / out_status; NULL ctx; NULL cloud_off_dev or
 * jobs_dev.  More than INT32_MAX points in a cloud or 2^28 in a job: ROMAN_E_TOO_LARGE.
 */
#define ROMAN_INTEGRATE_NEIGHBORS 10
#define ROMAN_INTEGRATE_WAVE_MAX  256   /* a job of at most so many points (base + added) is one wave's (roman_ctx_set_integrate_cuts) */
#define ROMAN_INTEGRATE_LDS_MAX  4096   /* ... of at most so many is sorted by one workgroup in LDS; larger jobs merge through global memory */
typedef struct roman_integrate_params {
    double  voxel_size;        /* > 0, finite (segment_voxel_size) */
    double  outlier_std;       /* segment_outlier_removal_std; not finite or <= 0: no outlier removal */
    int32_t nb_neighbors;      /* ROMAN_INTEGRATE_NEIGHBORS; any other value is refused */
} roman_integrate_params_t;
typedef struct roman_integrate_job {
    int32_t base;              /* cloud of the segment, -1: a new segment */
    int32_t add;               /* cloud that is added */
    int32_t pose;              /* pose of the added cloud, -1: it is in the world frame already */
} roman_integrate_job_t;
ROMAN_API int roman_segment_integrate_dev(roman_ctx_t* ctx, const roman_integrate_params_t* params, const double* points, const int64_t* cloud_off_dev,
                                          const int64_t* cloud_off_host, int32_t n_clouds, const double* poses, int32_t n_poses,
                                          const roman_integrate_job_t* jobs_dev, const roman_integrate_job_t* jobs_host, int32_t n_jobs,
                                          double* out_points, int32_t* out_count, int32_t* out_status, double* out_avg, double* out_thr);

/* The same with HOST pointers everywhere.  Synchronous.  What a job leaves untouched comes back as the caller had it. */
ROMAN_API int roman_segment_integrate(roman_ctx_t* ctx, const roman_integrate_params_t* params, const double* points, const int64_t* cloud_off, int32_t n_clouds,
                                      const double* poses, int32_t n_poses, const roman_integrate_job_t* jobs, int32_t n_jobs,
                                      double* out_points, int32_t* out_count, int32_t* out_status, double* out_avg, double* out_thr);

/* Measurement only: the two point counts (base + added) at which a job of roman_segment_integrate* changes its kernel set — up to
   wave_max one wave, up to lds_max one workgroup sorting in LDS, beyond it one workgroup that sorts chunks of lds_max pairs and merges
   them in global memory.  0: the default again (ROMAN_INTEGRATE_WAVE_MAX, ROMAN_INTEGRATE_LDS_MAX); wave_max <= lds_max,
   2 <= lds_max <= 4096.  Every class gives the same bits, so results do not depend on the cuts. */
ROMAN_API int roman_ctx_set_integrate_cuts(roman_ctx_t* ctx, int32_t wave_max, int32_t lds_max);

/*
 * roman_segment_cluster_dev: what the mapper does to a segment that goes inactive — Segment.final_cleanup
 * [REF roman/object/segment.py:195-220], called with clustering_epsilon when a segment has not been seen for max_t_no_sightings
 * [REF roman/map/mapper.py:92-105]: open3d's cluster_dbscan(eps, min_points) over the segment's cloud, then "keep the largest
 * cluster".  One call takes a LIST OF JOBS, one per segment going inactive.  Bulk data on the DEVICE; a PURE ENQUEUE on the
 * context's stream: no synchronisation, no read-back.
 *   params          roman_cluster_params_t, below
 *   points          float64[P][3]: n_clouds clouds one behind the other, P = cloud_off_host[n_clouds] [REF roman/object/segment.py:203-205]
 *   cloud_off_dev   int64[n_clouds + 1] on the device, cloud_off_host the same numbers on the HOST: ascending, [0] == 0
 *   jobs_dev        int32[n_jobs] on the device, jobs_host the same on the HOST: the cloud of every job — the segments of
 *                   to_rm [REF roman/map/mapper.py:93-95].  A cloud is named by at most one job
 *   SLOTS           job j owns the elements [slot_j, slot_j + n(cloud_j)) of out_points and out_labels, slot_j the exclusive
 *                   prefix sum of the point counts of the jobs in front of it, computed from cloud_off_host alone; all workspace
 *                   is laid out the same way, and no write of a job leaves its slot
 *   out_points      float64[total][3]: the first out_count[j] rows of slot j are the kept cluster's points in INPUT ORDER
 *                   [REF roman/object/segment.py:217-218]; the rest of the slot is left untouched.  May be NULL when total == 0
 *   out_count       int32[n_jobs]: 0 with n_clusters == 0 is the case in which the reference's np.argmax raises
 *                   [REF roman/object/segment.py:211-214] and the mapper's except branch drops the segment [REF roman/map/mapper.py:97-105]
 *   out_status      int32[n_jobs], the vocabulary of roman_assoc_scores: ROMAN_ASSOC_OK; ROMAN_ASSOC_EMPTY: the cloud holds no
 *                   point (the reference does nothing to points = None [REF roman/object/segment.py:203]), count 0;
 *                   ROMAN_ASSOC_RANGE: a coordinate is not finite — count 0, the slot of out_labels untouched.  Both write
 *                   n_clusters 0 and kept -1
 *   out_labels      int32[total] or NULL: open3d's label of every input point [REF roman/object/segment.py:205], -1: noise
 *   out_n_clusters  int32[n_jobs]: max(label) + 1 [REF roman/object/segment.py:208-211]
 *   out_kept        int32[n_jobs] or NULL: the label of the kept cluster [REF roman/object/segment.py:214], -1 when there is none
 *   NO ALIASING     the rule of roman_segment_integrate_dev: no output may overlap points, cloud_off, jobs or another output
 * Semantics (tests/_dbscan_oracle.py states them twice: open3d's loop literally, and the closed form below; a CPU test holds one
 * to the other).  open3d is not compared with: three things are UNPINNED.  (1) THE ROUNDING OF d2: d2(i, j) = (dx dx + dy dy) +
 * dz dz in double without contraction, the expression of roman_segment_integrate_dev.  (2) THE STRICT RADIUS COMPARISON: j is a
 * neighbour of i iff d2 < eps eps (nanoflann's radius result set), eps eps formed once in double; every point is its own
 * neighbour and the relation is symmetric bit for bit.  (3) THE CLOSED FORM OF THE LABEL ORDER: i is a core point iff it has at
 * least min_points neighbours, itself included; clusters are the connected components of the core points under the neighbour
 * relation, labelled 0, 1, ... in ascending order of their smallest core index; a non-core point with a core neighbour takes the
 * smallest label among its core neighbours, one without is noise (-1) — what open3d's sequential loop (outer index ascending, a
 * cluster expanded fully before the next, noise relabelled by a later cluster that reaches it) arrives at.  Then final_cleanup:
 * sizes count core and border members; the largest cluster is kept, among equals the lowest label (np.argmax).  Integer atomics
 * only, and the roots of the union-find do not depend on the schedule: two calls give the same bytes, and so does every size
 * class.  n_jobs == 0: ROMAN_OK, nothing written.
 * Errors (ROMAN_E_INVALID with a roman_last_error text, nothing enqueued; the argument checks run before the context is looked
 * at): NULL params; eps not finite or <= 0; min_points < 1; a negative count; NULL cloud_off_host, [0] != 0 or descending; NULL
 * jobs_host; a job out of range; a cloud named twice; NULL points with P > 0; NULL out_points / out_count / out_status /
 * out_n_clusters; NULL ctx; NULL cloud_off_dev or jobs_dev.  More than INT32_MAX points in a cloud or 2^28 in the call:
 * ROMAN_E_TOO_LARGE.
 */
#define ROMAN_CLUSTER_MIN_POINTS 10     /* final_cleanup's default [REF roman/object/segment.py:195] */
#define ROMAN_CLUSTER_WAVE_MAX  256     /* a job of at most so many points is one wave's (roman_ctx_set_cluster_cuts) */
#define ROMAN_CLUSTER_LDS_MAX  1536     /* ... of at most so many is one workgroup's, resident in LDS; larger jobs are tiled through global memory */
#define ROMAN_CLUSTER_TILE      256     /* query points of one workgroup of the tiled class */
#define ROMAN_CLUSTER_COLS     1024     /* column points the tiled class stages in LDS at a time */
typedef struct roman_cluster_params {
    double  eps;          /* clustering_epsilon [REF roman/params/mapper_params.py:68]; finite, > 0 */
    int32_t min_points;   /* final_cleanup's default 10 [REF roman/object/segment.py:195]; >= 1; a RUN-TIME value */
} roman_cluster_params_t;
ROMAN_API int roman_segment_cluster_dev(roman_ctx_t* ctx, const roman_cluster_params_t* params, const double* points, const int64_t* cloud_off_dev,
                                        const int64_t* cloud_off_host, int32_t n_clouds, const int32_t* jobs_dev, const int32_t* jobs_host, int32_t n_jobs,
                                        double* out_points, int32_t* out_count, int32_t* out_status, int32_t* out_labels, int32_t* out_n_clusters,
                                        int32_t* out_kept);

/* The same with HOST pointers everywhere.  Synchronous.  What a job leaves untouched comes back as the caller had it. */
ROMAN_API int roman_segment_cluster(roman_ctx_t* ctx, const roman_cluster_params_t* params, const double* points, const int64_t* cloud_off, int32_t n_clouds,
                                    const int32_t* jobs, int32_t n_jobs, double* out_points, int32_t* out_count, int32_t* out_status,
                                    int32_t* out_labels, int32_t* out_n_clusters, int32_t* out_kept);

/* Measurement and tests only: the two point counts at which a job of roman_segment_cluster* changes its kernel set — up to wave_max
   one wave, up to lds_max one workgroup with the job resident in LDS, beyond it (job, query tile) workgroups through global memory.
   0: the default again (ROMAN_CLUSTER_WAVE_MAX, ROMAN_CLUSTER_LDS_MAX); wave_max <= 256, wave_max <= lds_max, 1 <= lds_max <= 1536.
   Every class gives the same bytes, so results do not depend on the cuts. */
ROMAN_API int roman_ctx_set_cluster_cuts(roman_ctx_t* ctx, int32_t wave_max, int32_t lds_max);

/*
 * roman_session_gate_aabb_dev: roman_session_gate_dev with the bounding-box gate [REF roman/align/submap_align.py:101-103]
 * — what roman_grid_gate_aabb_dev is to roman_grid_gate_dev.  The arguments are roman_session_gate_dev's; then
 *   box        float64[S][6] over ALL submaps of the session, as roman_session_boxes_dev wrote them.  NEARBY is the six comparisons
 *              of [REF roman/utils.py:167-169] on box[gi] and box[gj], <= and >= as they stand: touching boxes intersect, an empty
 *              submap's box intersects nothing.  gparams->radius is NOT read (any value, NaN included)
 *   sim_in     float64[pair_off[nb]] or NULL.  Given: the similarity of every pair is already there (roman_session_stacked_sim_dev's),
 *              read as roman_session_gate_sim_dev reads it and never written; gparams->desc_dim must then be 0 (ROMAN_E_INVALID
 *              otherwise), `desc` is not read and `sim` is not written (both may be NULL)
 * Per block every output is bit for bit what roman_grid_gate_aabb_dev writes for the block's two sides (pairs after re-basing).
 * Everything else is roman_session_gate_dev's contract: the tables and their validation, the compact list by a prefix sum (no
 * atomics), todo_off, the slots beyond todo_off[nb] untouched, the errors — without those of the radius, plus box NULL while a
 * pair exists -> ROMAN_E_INVALID.
 */
ROMAN_API int roman_session_gate_aabb_dev(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                                          const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                          int32_t nb, const int32_t* blocks, const int32_t* blocks_host,
                                          const int64_t* pair_off, const int64_t* pair_off_host, const int64_t* tile_off, const int64_t* tile_off_host,
                                          double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                          int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* box, const double* sim_in);

/* The same with HOST pointers everywhere (each table once).  Synchronous; box and sim_in go up and are not brought back (sim comes
   back only without sim_in).  The caller's pairs, T_ref and enable go up first: the slots beyond todo_off[nb] come back as they were. */
ROMAN_API int roman_session_gate_aabb(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                                      const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                      int32_t nb, const int32_t* blocks, const int64_t* pair_off, const int64_t* tile_off,
                                      double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                      int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off, const double* box, const double* sim_in);

/*
 * roman_session_gate_list_dev: pass 1 of a session for an explicit LIST of pairs instead of whole robot-pair
 * grids — what a session that grows asks for: only the pairs a new or changed submap touches.  R, sub_off, pos, pos_gt, has_gt,
 * T_w, time, desc, nb, blocks and pair_off are roman_session_gate_dev's, validated as there and in front of everything else (no
 * tile_off: the list is the work).  Every bulk pointer DEVICE; a PURE ENQUEUE on the context's stream; the small tables and the
 * list travel twice (device, and `_host` copies the library validates).
 *
 *   L, list    int32[L][3]: (b, i, j) — block index, block-local row and column.  Strictly ascending in (b, i, j): no pair twice
 *   box        float64[S][6] or NULL.  Given: the bounding-box gate, roman_session_gate_aabb_dev's rules; the radius is not read
 *   sim_in     float64[pair_off[nb]] or NULL.  Given: the similarity of every pair of every block is already there, at the pair's
 *              DENSE position pair_off[b] + i * n1 + j (roman_session_stacked_sim_dev's layout), gated by roman_session_gate_sim_dev's
 *              rules: gparams->desc_dim must be 0, equality with the threshold passes; `desc` is not read
 *
 * Outputs per LISTED pair (L entries, in list order): dist, flags, yaw_deg, sim, T_ij (x16) — entry l bit for bit what
 * roman_session_gate_dev (roman_session_gate_sim_dev / _aabb_dev) writes at that pair's dense position over the same tables; with
 * sim_in, sim[l] is the copy of the pair's entry of sim_in.  Compact outputs (capacity L; slots beyond the total untouched):
 * pairs (GLOBAL gi, gj), T_ref, enable, and todo_off int32[nb+1] — the TODO pairs in list order, block b's in the slots
 * [todo_off[b], todo_off[b+1]).  With the full list (every pair of every block) every output equals the whole-grid call's.
 * No atomics: two runs agree bit for bit.
 *
 * L == 0: ROMAN_OK, todo_off all 0, nothing else written.  Errors: roman_session_gate_dev's about its tables and gparams; L < 0, a
 * NULL list with L > 0, an entry with b outside [0, nb) or (i, j) outside its block, a list not strictly ascending, sim_in with
 * desc_dim != 0, a NULL output that is needed -> ROMAN_E_INVALID; L * 16 beyond int32 -> ROMAN_E_TOO_LARGE.
 */
ROMAN_API int roman_session_gate_list_dev(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off, const int32_t* sub_off_host,
                                          const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                          int32_t nb, const int32_t* blocks, const int32_t* blocks_host, const int64_t* pair_off, const int64_t* pair_off_host,
                                          int32_t L, const int32_t* list, const int32_t* list_host, const double* box, const double* sim_in,
                                          double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                          int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off);

/* The same with HOST pointers everywhere (each table and the list once).  Synchronous; box and sim_in go up and are not brought
   back.  The caller's pairs, T_ref and enable go up first: the slots beyond todo_off[nb] come back as they were. */
ROMAN_API int roman_session_gate_list(roman_ctx_t* ctx, const roman_grid_gate_params_t* gparams, int32_t R, const int32_t* sub_off,
                                      const double* pos, const double* pos_gt, const int32_t* has_gt, const double* T_w, const double* time, const double* desc,
                                      int32_t nb, const int32_t* blocks, const int64_t* pair_off, int32_t L, const int32_t* list, const double* box, const double* sim_in,
                                      double* dist, int32_t* flags, double* yaw_deg, double* sim, double* T_ij,
                                      int32_t* pairs, double* T_ref, int32_t* enable, int32_t* todo_off);

/* ------------------------------------------------------------------------------------------- */
/* stepwise surface for the clipperpy-compatible shim (single problem, host pointers)          */
/* ------------------------------------------------------------------------------------------- */

/* clipperpy.utils.create_all_to_all(n1, n2) [REF roman/align/object_registration.py:41]:
   out is (n1*n2, 2) int32, row i*n2+j = (i, j).  Pure host helper. */
ROMAN_API int roman_create_all_to_all(int32_t n1, int32_t n2, int32_t* out);

/* score_pairwise_consistency / score_pairwise_and_single_consistency
   [REF roman/align/object_registration.py:47], [REF roman/align/roman_registration.py:95]:
   builds M (and C, which has M's pattern) for ONE problem on the device and keeps it in the
   context.  assoc may be NULL, or n_assoc 0 (all-to-all). */
ROMAN_API int roman_score(roman_ctx_t* ctx, const roman_params_t* params,
                const double* D1, int32_t n1, const double* D2, int32_t n2, int32_t F,
                const int32_t* assoc, int32_t n_assoc);

/* clipper.set_matrix_data(M=, C=) [REF roman/align/object_registration.py:64]: dense
   row-major (n,n) float64 M and C; like upstream only the strict upper triangles are used
   and the diagonal is the implicit identity.  M and C are uploaded and converted to the
   solver's layout on the device (host pointers in, two small read-backs); the matrices stay
   in the context. */
ROMAN_API int roman_set_matrix_data(roman_ctx_t* ctx, const roman_params_t* params,
                          const double* M, const double* C, int32_t n);

/* clipper.solve() [REF roman/align/object_registration.py:27,65] on the matrices held by
   the context.  u0 may be NULL (all ones). */
ROMAN_API int roman_solve(roman_ctx_t* ctx, const double* u0);

/* Size queries + getters for the last roman_score/roman_set_matrix_data/roman_solve. */
ROMAN_API int roman_num_associations(const roman_ctx_t* ctx, int32_t* n_assoc);       /* rows of A     */
ROMAN_API int roman_num_selected(const roman_ctx_t* ctx, int32_t* n_sel);             /* len(nodes)    */
/* clipper.get_selected_associations() [REF object_registration.py:28]: (n_sel,2) int32 */
ROMAN_API int roman_get_selected_associations(const roman_ctx_t* ctx, int32_t* out);
/* clipper.get_solution().nodes / .u / .score [REF object_registration.py:67-71] */
ROMAN_API int roman_get_solution(const roman_ctx_t* ctx, int32_t* nodes, double* u, double* score,
                       roman_stats_t* stats);
/* clipper.get_affinity_matrix() / get_constraint_matrix() [REF object_registration.py:53-54]:
   dense row-major (A,A) float64, symmetric, diagonal included (1 for EUCLIDEAN, the single
   score for ROMAN; C's diagonal is 1).  Caller provides A*A doubles each; either may be NULL. */
ROMAN_API int roman_get_dense_matrices(const roman_ctx_t* ctx, double* M, double* C);
/* Sparse export of the same (strict upper triangle, CSR over association indices, ascending
   columns) for tests: call with NULL arrays to get nnz first. */
ROMAN_API int roman_get_upper_csr(const roman_ctx_t* ctx, int64_t* nnz, int64_t* rowptr /*A+1*/,
                        int32_t* cols, double* vals, double* diag /*A*/);

/* ------------------------------------------------------------------------------------------- */
/* pose from given correspondences                                                             */
/* ------------------------------------------------------------------------------------------- */

/* ObjectRegistration.T_align(map1, map2, correspondences) [REF object_registration.py:88-129]
   for B independent correspondence sets, host pointers.  pts1/pts2: (sum k_b, dim) float64
   row-major already gathered point pairs ([REF :110-111]); corr_off: int64[B+1].
   T_out: B x 16 doubles; status_out: ROMAN_ST_INSUFFICIENT when k_b < dim ([REF :107-108]). */
ROMAN_API int roman_pose_batch(roman_ctx_t* ctx, int32_t dim, int32_t B,
                     const double* pts1, const double* pts2, const int64_t* corr_off,
                     double* T_out, int32_t* status_out);

/* ------------------------------------------------------------------------------------------- */
/* instrumentation                                                                             */
/* ------------------------------------------------------------------------------------------- */

/* When enabled, the batch call brackets each of its kernels with hipEvents on the context's
   stream; roman_profile_get returns the accumulated per-stage milliseconds and launch counts
   since the last roman_profile_reset.  Stage ids: */
#define ROMAN_STAGE_SINGLE   0   /* norms, cos-sim MFMA GEMM, distance tables, single scores + live compaction */
#define ROMAN_STAGE_COUNT_PASS 1 /* affinity pair tests, mirror, degree sort, candidate lists, problem scans   */
#define ROMAN_STAGE_FILL     2   /* affinity fill: candidate lists -> matrix values                            */
#define ROMAN_STAGE_SOLVE    3   /* persistent projected-gradient solvers (+ select + pose)                    */
#define ROMAN_STAGE_COUNT    4
ROMAN_API int roman_profile_enable(roman_ctx_t* ctx, int on);
ROMAN_API int roman_profile_reset(roman_ctx_t* ctx);
ROMAN_API int roman_profile_get(roman_ctx_t* ctx, double ms[ROMAN_STAGE_COUNT],
                      int64_t launches[ROMAN_STAGE_COUNT]);

/* Diagnostics for tests: evaluate a device math primitive elementwise (host pointers).
   kind 0: sqrt(x)  1: exp(x)  2: cbrt(x)  3: x/y (y = in2)  4: pow(x,y)  5: the library's fixed-sequence
   exp  6: its fixed-sequence cbrt  7: fma(x,y,x).  Used to check that the device's +,-,*,/,sqrt,fma and the
   two fixed-sequence functions are bit-identical to the host's (pattern parity) and to
   measure the ulp distance of the device's libm. */
ROMAN_API int roman_debug_math(roman_ctx_t* ctx, int kind, const double* in1, const double* in2,
                     int64_t n, double* out);
/* Diagnostics for tests: normalised cosine matrix (n1 x n2, row-major) of the cosine-feature
   blocks of two object-major feature matrices, computed by the f64 MFMA kernel of stage SINGLE. */
ROMAN_API int roman_debug_cosine(roman_ctx_t* ctx, const roman_params_t* params,
                       const double* D1, int32_t n1, const double* D2, int32_t n2, int32_t F,
                       double* out);
/* Diagnostics for tests: live association list of the last roman_score (original association
   index and single score of every live association, ascending). n_live via roman_get_solution
   stats or by calling with NULL arrays. */
ROMAN_API int roman_debug_live(const roman_ctx_t* ctx, int32_t* n_live, int32_t* idx, double* score);

/* Library build info: "roman_hip <version> gfx950 ..." */
ROMAN_API const char* roman_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ROMAN_HIP_H */
