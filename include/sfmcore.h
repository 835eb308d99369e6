/*
 * sfmcore.h — C-ABI of the MI355X-native bundle-adjustment and descriptor
 * matching core (libsfmcore.so).
 *
 * This is the drop-in boundary for the two hot paths of
 * RainbowXXX/3DReconstruction (reference tree, read-only):
 *
 *   BA   : src/adjuster/BundleAdjuster.h:100-141  (ceres::Solve over the
 *          whole WorldStructure; ReprojectCost :33-69, HuberLoss(4) :109,
 *          gauge :105, options :167-174, write-back :143-156)
 *   Match: src/sparseBuilder/sparseBuilder.cpp:758-807 (matchPair,
 *          exhaustive pairs) and :809-1023 (match, Matcher_Regions(0.8,
 *          BRUTE_FORCE_L2) :919-921), plus the legacy exact matcher
 *          src/frame/LocalFrame.h:31-47 / GlobalFrame.h:22-43
 *          (cv::BFMatcher(NORM_L2, crossCheck) knnMatch k=1).
 *
 * Conventions
 *   - Plain pointers and sizes only; every buffer is caller owned.  No
 *     allocation crosses the ABI.  Nothing here throws.
 *   - Every function returns 0 (SFM_OK) on success or a negative SFM_ERR_*
 *     code; sfm_last_error() returns a thread-local message for the last
 *     failure on the calling thread.
 *   - One sfm_ctx per thread (contexts are independent; a context is not
 *     re-entrant).  A context owns its HIP device, stream(s) and, when
 *     world_size > 1, an RCCL communicator over xGMI.
 *   - Functions marked [cpu] never touch the GPU and work without one.
 */
#ifndef SFMCORE_H
#define SFMCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the C-ABI is the only exported surface (libraries build with hidden default visibility) */
#pragma GCC visibility push(default)

#define SFM_OK                 0
#define SFM_ERR_INVALID_ARG   -1
#define SFM_ERR_DEVICE        -2   /* HIP runtime error / no gfx950 device      */
#define SFM_ERR_NOT_FINITE    -3   /* non-finite residual at the initial point   */
#define SFM_ERR_UNSUPPORTED   -4   /* problem shape outside this build's kernels */
#define SFM_ERR_COMM          -5   /* RCCL failure                               */
#define SFM_ERR_OOM           -6
#define SFM_ERR_SOLVER        -7   /* LM terminated with FAILURE (not usable)    */

/* [cpu] library identification and last error message (thread local). */
const char* sfm_version(void);
const char* sfm_last_error(void);

/* ------------------------------------------------------------------------ */
/* Context                                                                   */
/* ------------------------------------------------------------------------ */
typedef struct sfm_ctx sfm_ctx;

/* Host-side all-reduce hook: reduce buf[n] across all ranks in place,
 * op 0 = sum, 1 = max; return 0 on success. */
typedef int32_t (*sfm_allreduce_fn)(void* user, double* buf, int64_t n, int32_t op);

typedef struct sfm_ctx_opts {
    int32_t device;          /* HIP device ordinal (local to the process)      */
    int32_t rank;            /* 0 .. world_size-1                              */
    int32_t world_size;      /* 1 = single GPU; >1 = landmark-sharded BA       */
    int32_t flags;           /* SFM_CTX_* bits (0 = defaults)                  */
    const uint8_t* comm_id;  /* 128-byte RCCL unique id from rank 0's
                                sfm_comm_unique_id(); NULL when world_size==1
                                or when `allreduce` is given (at world_size 1
                                it builds a 1-rank communicator: the RCCL
                                exchanges run and are identities)             */
    sfm_allreduce_fn allreduce; /* optional (world_size > 1, comm_id NULL):
                                the per-iteration exchanges are staged through
                                pinned host memory and handed to this hook
                                (MPI, gloo, ...) instead of RCCL over xGMI   */
    void* allreduce_user;
} sfm_ctx_opts;

/* sfm_ctx_opts.flags.  SFM_CTX_TUNE_HOST_MALLOC (opt-in): keep freed host memory in
 * the process heap (glibc M_MMAP_THRESHOLD at its 32 MiB maximum, and
 * M_TRIM_THRESHOLD).  Unmapping a large host buffer stalls the process's next
 * GPU operation for 10-30 ms while the driver invalidates its mappings, which
 * an incremental loop (BA, then matching, per image) pays every step; the
 * price is that the heap does not shrink, so a long-running host application
 * leaves it off (the default: its malloc settings are not touched). */
#define SFM_CTX_TUNE_HOST_MALLOC 1
/* Diagnostic only: world_size > 1 with every exchange a no-op (no RCCL, no
 * hook).  The context plans and runs rank `rank`'s landmark shard alone, so
 * its kernels and wall time are what that rank spends in an N-GPU run minus
 * the collectives; the solve is not the global one (bench.py --fake-world). */
#define SFM_CTX_DIAG_NO_EXCHANGE 2
/* Diagnostic only (error-path tests): every reduced-camera-system solve of
 * this context reports that one of its dataflow waits timed out, as when
 * another context holds the CUs a persistent solve kernel needs.  The solve
 * verdict is max-reduced over ranks with the other per-iteration maxima, so
 * every rank of a sharded solve then returns SFM_ERR_DEVICE together instead
 * of the others waiting in the next collective. */
#define SFM_CTX_DIAG_FAIL_SOLVE_WAIT 4
/* Measurement: sfm_fmatrix_ac, sfm_triangulate, sfm_tracks_build, sfm_resect and sfm_relpose bracket their kernels with
 * HIP events (after draining the uploads) so that sfm_ctx_last_kernel_ms can
 * report the kernels alone.  Off by default: the extra stream synchronisation and event pair are
 * not part of the filter's production path. */
#define SFM_CTX_TIME_KERNELS 8
/* Diagnostic only (tests): the device's copy of the LM accept decision is
 * forced to "accept", so the speculative Gram pass at the candidate runs after
 * every step and the host has to redo it at the current point for each step
 * it rejects (the path a device / host disagreement would take). */
#define SFM_CTX_DIAG_SPEC_ALWAYS (1 << 11)
/* BA engine shape (A/B measurement and tests; 0 = the measured defaults).
 * Every alternative is exact: the launch-shape bits and the per-point /
 * per-target lane counts change only how the same sums are launched
 * (bit-identical results, or sums in another fixed order), the solver bits
 * pick the other direct solver of the same reduced camera system.  They are
 * read when a plan is created (sfm_ba_plan_create, sfm_ba_solve); there are
 * no environment switches for any of them.
 *   SFM_CTX_BA_DENSE_RCS     blocked dense Cholesky even for a narrow band
 *   SFM_CTX_BA_SEQ_BAND      the sequential block-band solver instead of
 *                            cyclic reduction (4-wide intrinsics arrows)
 *   SFM_CTX_BA_TILE80        80-row Schur tiles for every chunk
 *   SFM_CTX_BA_SPLIT_REDUCE  the RCS reduction in three launches (short
 *                            targets, long-target segments, their combine)
 *   SFM_CTX_BA_SPLIT_BCR     cyclic reduction's top, corner and every
 *                            back-substitution level as separate launches
 *   SFM_CTX_BA_DENSE_CHAIN   the dense factorisation and back substitution
 *                            as launch chains instead of dataflow kernels
 *   SFM_CTX_BA_NO_SPEC_GRAM  the Gram pass after an accepted step launched by
 *                            the host after its decision, not speculatively
 *   SFM_CTX_BA_STEP_LANES(n) n = 1, 2, 4, 8 lanes per point in the step pass
 *   SFM_CTX_BA_REDUCE_WAVES(n) n = 1, 2, 4 waves per reduce target
 * (a field of 0 means the planner's default; any other n gives the field
 * value 7, which sfm_ctx_create rejects with SFM_ERR_INVALID_ARG) */
#define SFM_CTX_BA_DENSE_RCS      (1 << 4)
#define SFM_CTX_BA_SEQ_BAND       (1 << 5)
#define SFM_CTX_BA_TILE80         (1 << 6)
#define SFM_CTX_BA_SPLIT_REDUCE   (1 << 7)
#define SFM_CTX_BA_SPLIT_BCR      (1 << 8)
#define SFM_CTX_BA_DENSE_CHAIN    (1 << 9)
#define SFM_CTX_BA_NO_SPEC_GRAM   (1 << 10)
#define SFM_CTX_BA_STEP_LANES(n)  (((n) == 8 ? 4 : (n) == 4 ? 3 : (n) == 2 ? 2 : (n) == 1 ? 1 : 7) << 12)
#define SFM_CTX_BA_REDUCE_WAVES(n) (((n) == 4 ? 3 : (n) == 2 ? 2 : (n) == 1 ? 1 : 7) << 15)

/* [cpu] fill out[128] with a fresh RCCL unique id (rank 0 only). */
int sfm_comm_unique_id(uint8_t* out128);
int sfm_ctx_create(const sfm_ctx_opts* opts, sfm_ctx** out);
int sfm_ctx_destroy(sfm_ctx* ctx);
int sfm_ctx_synchronize(sfm_ctx* ctx);

/* ------------------------------------------------------------------------ */
/* Bundle adjustment                                                         */
/*                                                                          */
/* Residual (BundleAdjuster.h:40-65): P = R(w) X + t (ceres::AngleAxisRotate- */
/* Point), u = fx P0/P2 + cx, v = fy P1/P2 + cy, r = (u - obs.x, v - obs.y).   */
/* Parameter blocks: extr[6*n_img] = {w0,w1,w2,t0,t1,t2} per image,          */
/* intr[4*n_intr] = {fx,fy,cx,cy} (camera_model selects others), X[3*n_pt].   */
/* Loss HuberLoss(huber_a).                                                  */
/* ------------------------------------------------------------------------ */
typedef struct sfm_ba_problem {
    int32_t n_img;           /* posed images (extrinsic blocks)                */
    int32_t n_intr;          /* intrinsic blocks (Camera objects)              */
    int64_t n_pt;            /* world points                                   */
    int64_t n_obs;           /* observations = residual blocks                 */
    const int64_t* pt_offsets;/* [n_pt+1] landmark-major: obs of point p are
                                 pt_offsets[p] .. pt_offsets[p+1]-1          */
    const int32_t* obs_img;  /* [n_obs] image of each observation              */
    const double*  obs_uv;   /* [2*n_obs] observed pixel (x, y)                */
    const int32_t* img_intr; /* [n_img] intrinsic block of each image          */
    int32_t const_img;       /* gauge: image whose pose is held constant
                                (BundleAdjuster.h:105); -1 for none          */
    int32_t camera_model;    /* SFM_CAM_* residual model (0 = the reference's
                                ReprojectCost)                               */
    double huber_a;          /* HuberLoss scale a (reference: 4.0); <=0: none  */
} sfm_ba_problem;

/* Residual models (sfm_ba_problem.camera_model).  The intrinsics blocks of
 * intr[] are 4 doubles wide, except RADIAL3's 6 (sfm_ba_intr_width()):
 *   SFM_CAM_PINHOLE  BundleAdjuster.h:33-69 ReprojectCost, {fx, fy, cx, cy}:
 *                    r = (fx P0/P2 + cx - u, fy P1/P2 + cy - v)
 *   SFM_CAM_SNAVELY  src/adjuster/SnavelyReprojectionError.h:16-54 (BAL /
 *                    Bundler), {f, l1, l2, -}: p = (-P0/P2, -P1/P2),
 *                    r = f (1 + |p|^2 (l1 + l2 |p|^2)) p - (u, v); the 4th
 *                    double is not a parameter (never read, never moved).
 *   SFM_CAM_RADIAL3  OpenMVG Pinhole_Intrinsic_Radial_K3 with ADJUST_ALL, as
 *                    reconstruction() selects it (sparseBuilder.cpp:1292-1299;
 *                    ResidualErrorFunctor_Pinhole_Intrinsic_Radial_K3),
 *                    {f, ppx, ppy, k1, k2, k3}: x = P0/P2, y = P1/P2,
 *                    c = 1 + k1 r2 + k2 r2^2 + k3 r2^3 (r2 = x^2 + y^2),
 *                    r = (ppx + f x c - u, ppy + f y c - v).  Solved through
 *                    the general-point path and the dense reduced camera
 *                    system. */
#define SFM_CAM_PINHOLE 0
#define SFM_CAM_SNAVELY 1
#define SFM_CAM_RADIAL3 2
/* [cpu] doubles per intrinsics block of a model (4, or 6 for RADIAL3);
 * 0 for an unknown model. */
int sfm_ba_intr_width(int32_t camera_model);

typedef struct sfm_ba_options {  /* ceres::Solver::Options semantics      */
    int32_t max_num_iterations;            /* 50   */
    int32_t max_num_consecutive_invalid_steps; /* 5 */
    int32_t jacobi_scaling;                /* 1    */
    int32_t reserved;
    double function_tolerance;             /* 1e-6 */
    double gradient_tolerance;             /* 1e-10 */
    double parameter_tolerance;            /* 1e-8 */
    double initial_trust_region_radius;    /* 1e4  */
    double max_trust_region_radius;        /* 1e16 */
    double min_trust_region_radius;        /* 1e-32 */
    double min_relative_decrease;          /* 1e-3 */
    double min_lm_diagonal;                /* 1e-6 */
    double max_lm_diagonal;                /* 1e32 */
} sfm_ba_options;

/* ceres::TerminationType subset */
#define SFM_TERM_CONVERGENCE     0
#define SFM_TERM_NO_CONVERGENCE  1
#define SFM_TERM_FAILURE         2

typedef struct sfm_ba_summary {
    double initial_cost;     /* 1/2 sum rho(|r|^2) at the input parameters     */
    double final_cost;
    int64_t num_residuals;   /* 2 * n_obs                                      */
    int32_t iterations;      /* ceres summary.iterations.size()-1 (iteration 0
                                is the initial evaluation)                    */
    int32_t successful_steps;/* counts iteration 0, as Ceres does             */
    int32_t unsuccessful_steps;
    int32_t termination;     /* SFM_TERM_*                                     */
    int32_t usable;          /* summary.IsSolutionUsable()                     */
    int32_t reserved;
    double rmse_initial;     /* sqrt(initial_cost/num_residuals), the metric
                                BundleAdjuster.h:137 prints                  */
    double rmse_final;       /* sqrt(final_cost/num_residuals)  (:138)         */
    double seconds;          /* wall time of the LM loop                        */
} sfm_ba_summary;

/* One entry per minimizer iteration (ceres::IterationSummary subset); used to
 * compare accept/reject sequences between implementations. */
typedef struct sfm_ba_iter {
    int32_t iteration;
    int32_t step_is_valid;
    int32_t step_is_successful;
    int32_t reserved;
    double cost;
    double cost_change;
    double model_cost_change;
    double relative_decrease;
    double trust_region_radius;  /* radius after the iteration's update */
    double step_norm;
    double gradient_max_norm;
} sfm_ba_iter;

/* [cpu] Ceres defaults as used by BundleAdjuster() (BundleAdjuster.h:167-174). */
void sfm_ba_default_options(sfm_ba_options* opts);

/* One-shot: upload, solve, and (only if usable) write extr/intr/X back —
 * mirrors BundleAdjuster::operator() (BundleAdjuster.h:176-186).  With
 * world_size>1 every rank passes the full problem; each rank solves the
 * landmark shard sfm_ba_partition assigns it and writes back the cameras and
 * its own points only. */
int sfm_ba_solve(sfm_ctx* ctx, const sfm_ba_problem* prob,
                 double* extr, double* intr, double* X,
                 const sfm_ba_options* opts, sfm_ba_summary* summary);
/* sfm_ba_solve keeps its last plan in the context: a later call whose problem
 * has the same structure (n_*, pt_offsets, obs_img, img_intr, const_img,
 * camera_model -- compared exactly) reuses it and only uploads the new values
 * (a world that did not grow since the previous BundleAdjuster call,
 * SequentialActuator.h:226-229).  A call whose problem grows the cached one
 * (the same images, intrinsics map, gauge and model, with images, points and
 * observations only appended: every point keeps its observations in order
 * and may gain new ones at the end -- the next call of the incremental loop,
 * SequentialActuator.h:226-229 after addSingleImage, main.cpp:99-108) plans
 * only what the growth moved and takes the rest from the cached plan, with
 * the same result as a fresh plan bit for bit (world 1).  This releases that
 * plan (its device memory); sfm_ctx_destroy does too.  SFM_BA_NO_PLAN_CACHE=1
 * turns the cache off, SFM_BA_NO_GROWN_PLAN=1 the growth only. */
int sfm_ba_cache_clear(sfm_ctx* ctx);
/* [diagnostic] sfm_ba_solve calls on this context that reused the cached plan
 * as it was, grew it, or planned from scratch. */
int sfm_ba_cache_stats(sfm_ctx* ctx, int64_t* reused, int64_t* grown, int64_t* fresh);

/* Resident variant (used by the benchmark): the plan uploads the problem and
 * the initial parameters once; every sfm_ba_plan_run restarts from those
 * initial parameters with all data already in HBM. */
typedef struct sfm_ba_plan sfm_ba_plan;
int sfm_ba_plan_create(sfm_ctx* ctx, const sfm_ba_problem* prob,
                       const double* extr, const double* intr, const double* X,
                       sfm_ba_plan** out);
int sfm_ba_plan_run(sfm_ba_plan* plan, const sfm_ba_options* opts,
                    sfm_ba_summary* summary);
int sfm_ba_plan_download(sfm_ba_plan* plan, double* extr, double* intr, double* X);
int sfm_ba_plan_destroy(sfm_ba_plan* plan);

typedef struct sfm_ba_plan_info {
    int64_t shard_pt_begin, shard_pt_end;   /* rank's range in sorted order   */
    int64_t shard_obs;                      /* observations on this rank      */
    int32_t n_chunks;                       /* Schur work chunks              */
    int32_t band_blocks;                    /* block half-bandwidth D of S    */
    int32_t n_cam_active, n_intr_active;    /* RCS blocks                     */
    int64_t rcs_dim;                        /* 6*n_cam_active+w*n_intr_active */
    double  last_kernel_ms[8];              /* per-phase device time of the
                                               last iteration (HIP events)   */
    int64_t schur_flops_per_iter;           /* algorithmic flops, Schur kernel*/
    int64_t schur_launches;                 /* timed Schur launches, last run  */
    double  schur_ms_total;                 /* their summed kernel time (HIP
                                               events; only with the
                                               SFM_SCHUR_TIME_ALL diagnostic:
                                               an event pair serialises the
                                               stream, 0 launches otherwise) */
    int32_t rcs_solver;                     /* SFM_RCS_* the plan solves with  */
    int32_t tile_rows;                      /* Schur chunk tile height (64/80) */
} sfm_ba_plan_info;
/* sfm_ba_plan_info.rcs_solver */
#define SFM_RCS_BCR       0   /* block cyclic reduction of the band + arrow   */
#define SFM_RCS_DENSE     1   /* blocked dense Cholesky                      */
#define SFM_RCS_SEQ_BAND  2   /* sequential block-band Cholesky              */
int sfm_ba_plan_get_info(sfm_ba_plan* plan, sfm_ba_plan_info* info);
/* Iteration log of the last sfm_ba_plan_run (n <= cap entries written). */
int sfm_ba_plan_get_trace(sfm_ba_plan* plan, sfm_ba_iter* out, int32_t cap, int32_t* n);

/* [cpu] Structure the planner chooses for a problem (no device needed):
 * Schur chunks vs general points (any track length, repeated views, many
 * intrinsics blocks), camera half-bandwidth after ordering, and the reduced
 * camera system's form (dense = 1: blocked dense Cholesky; 0: block-banded
 * cyclic reduction). */
typedef struct sfm_ba_plan_shape {
    int32_t n_chunks, band_blocks, dense, n_cam_active, n_intr_active, tile_rows;
    int64_t n_chunk_pts, n_general_pts, rcs_dim, n_targets, n_terms, n_pterms;
} sfm_ba_plan_shape;
int sfm_ba_describe(const sfm_ba_problem* prob, int32_t rank, int32_t world_size, sfm_ba_plan_shape* out);

/* [cpu] Diagnostic (tests): plans `prob` twice -- from scratch, and grown
 * from the plan of `prev` (sfm_ba_solve's path when a problem extends the
 * previous call's: SequentialActuator::bundleAdjustment after
 * addSingleImage, src/actuator/SequentialActuator.h:226-229) -- and returns
 * the FNV-1a digest of every plan array the device reads in each (the
 * measurements excluded: a grown plan gathers them on the device).
 * *reused = the sorted points the grown plan took over from prev's plan, -1
 * when prob does not grow prev or prev's plan cannot seed it (digest_grown
 * then 0). */
int sfm_ba_grown_digest(const sfm_ba_problem* prev, const sfm_ba_problem* prob, uint64_t* digest_fresh,
                        uint64_t* digest_grown, int64_t* reused);

/* [cpu] Diagnostic (tests): the schedule of the dense RCS dataflow solve
 * (dense_flow_kernel) for `prob`'s plan, as the device reads it: permuted
 * tile order | previous column per chain | link / D / S bits | lookahead row
 * | chain 0 list | chain 1 list | the two lengths | tasks (kind << 24 | i << 12
 * | j, in execution order) | the tile pattern of L (nt * nt bytes).  Copies it
 * to out when *n_words <= cap (cap 0: size query).  shape[7] = {nt, chains,
 * tasks, 1 if the dataflow solve runs, nF, nb, camera half-bandwidth}; no schedule (n_words 0) for a
 * band problem or a system over the dataflow solve's size. */
int sfm_ba_dense_schedule(const sfm_ba_problem* prob, int32_t* out, int64_t cap, int64_t* n_words, int32_t* shape);

/* [cpu] Landmark-block partition: contiguous point ranges of the
 * (min-camera)-sorted point order with ~equal observation counts.
 * order[n_pt] receives the sorted point order, bounds[world_size+1] the
 * ranges into it. */
int sfm_ba_partition(const sfm_ba_problem* prob, int32_t world_size,
                     int64_t* order, int64_t* bounds);

/* [cpu] Deterministic synthetic scenes.  Two calls: first with
 * NULL arrays to get sizes, then with caller-allocated arrays.  vis_mode 0 =
 * banded orbit visibility (k consecutive cameras), 1 = random k cameras,
 * 2 = closed orbit (k consecutive cameras modulo n_cam).
 * gt_* receive ground truth, extr/intr/X the perturbed initial point. */
typedef struct sfm_synth_ba_config {
    int32_t n_cam, k, vis_mode, n_intr;   /* n_intr 1 = shared intrinsics      */
    int64_t n_pt;
    uint64_t seed;
    double noise_px, outlier_frac;        /* 0.5, 0.01                         */
    double perturb_rot, perturb_t, perturb_X, perturb_f; /* .01,.05,.05,5      */
    int32_t const_img;                    /* gauge (1)                          */
    int32_t camera_model;                 /* SFM_CAM_*; SNAVELY: f 1000,
                                             l1 -0.08, l2 0.02 (+ perturbation);
                                             RADIAL3: pinhole f / principal point,
                                             k1 -0.05, k2 0.01, k3 -0.002
                                             (intr / gt_intr 6 doubles a block) */
} sfm_synth_ba_config;
int sfm_synth_ba(const sfm_synth_ba_config* cfg,
                 int64_t* pt_offsets, int32_t* obs_img, double* obs_uv,
                 int32_t* img_intr, double* extr, double* intr, double* X,
                 double* gt_extr, double* gt_intr, double* gt_X,
                 int64_t* n_obs_out);

/* ------------------------------------------------------------------------ */
/* Descriptor matching (128-D uint8 SIFT/RootSIFT, exact integer L2^2)       */
/* ------------------------------------------------------------------------ */
#define SFM_MATCH_RATIO   0   /* Matcher_Regions(0.8, BRUTE_FORCE_L2): for each
                                 query j of image J, top-2 over image I; keep
                                 if d1 < fl32(ratio*ratio)*d2; emit (i, j)   */
#define SFM_MATCH_MUTUAL  1   /* BFMatcher(NORM_L2, crossCheck) knnMatch k=1:
                                 keep (i, j) iff j = NN_J(i) and i = NN_I(j) */
#define SFM_MATCH_CASCADE 2   /* Cascade_Hashing_Matcher_Regions(0.8), the
                                 "AUTO" default (sparseBuilder.cpp:811-814,
                                 911-914): per query j of J, candidates of I
                                 sharing one of 6 hash buckets, top-10 by
                                 Hamming distance re-ranked by exact L2^2,
                                 ratio test as RATIO; emit (i, j).  The
                                 zero-mean descriptor is taken over the
                                 images of the run's pair list.             */

typedef struct sfm_match_options {
    int32_t mode;            /* SFM_MATCH_*                                    */
    float ratio;             /* fDistRatio (sparseBuilder.cpp:812): 0.8f       */
} sfm_match_options;

/* Single image pair, dense output (behind LocalFrame/GlobalFrame::matchFeature).
 * Descriptors are row-major [n][128] uint8.  For RATIO the database is `a`
 * and the queries are `b` (OpenMVG: regions I vs queries J); for MUTUAL `a`
 * is the OpenCV query set and `b` the train set.  Outputs, per row of `b`
 * (RATIO) or per row of `a` (MUTUAL): the matched index in the other set or
 * -1, and the exact squared L2 distance of that match. */
int sfm_match_dense(sfm_ctx* ctx, const uint8_t* a, int32_t n_a,
                    const uint8_t* b, int32_t n_b,
                    const sfm_match_options* opts,
                    int32_t* match_idx, int32_t* match_d2);

/* The same with float descriptors: the cv::Mat CV_32F rows cv::SIFT gives
 * LocalFrame/GlobalFrame::matchFeature (src/frame/LocalFrame.h:38,
 * GlobalFrame.h:28-34, src/component/Image.h:39-41).  OpenCV's SIFT stores
 * saturate_cast<uchar> values in them, so rows whose every value is an
 * integer in [0, 255] are converted exactly and matched on the u8 path
 * (distances exact integers, < 2^24, hence exact floats).  Any other input is
 * matched in f32: d = sum_k (a_k - b_k)^2 accumulated as an fmaf chain in k
 * order (first minimum wins), bit for bit the oracle's restatement; OpenCV's
 * own SIMD summation order is not pinned for such input.  match_d2 is the
 * squared distance (DMatch.distance = sqrtf of it), -1 where unmatched. */
int sfm_match_dense_f32(sfm_ctx* ctx, const float* a, int32_t n_a,
                        const float* b, int32_t n_b,
                        const sfm_match_options* opts,
                        int32_t* match_idx, float* match_d2);

/* All-pairs matching over a resident descriptor collection. */
typedef struct sfm_match_plan sfm_match_plan;
/* desc: concatenated [sum n_img][128] uint8; desc_offsets[n_img+1]. */
int sfm_match_plan_create(sfm_ctx* ctx, const uint8_t* desc,
                          const int64_t* desc_offsets, int32_t n_img,
                          sfm_match_plan** out);
/* Float collection (the rules of sfm_match_dense_f32; SFM_MATCH_CASCADE
 * needs integer-valued descriptors and returns SFM_ERR_UNSUPPORTED
 * otherwise). */
int sfm_match_plan_create_f32(sfm_ctx* ctx, const float* desc,
                              const int64_t* desc_offsets, int32_t n_img,
                              sfm_match_plan** out);
/* pairs[2*n_pairs] = (I, J).  Results stay on the device. */
int sfm_match_plan_run(sfm_match_plan* plan, const int32_t* pairs,
                       int64_t n_pairs, const sfm_match_options* opts,
                       int64_t* total_matches);
/* SFM_MATCH_CASCADE tables (codes, buckets, zero-mean descriptor) for the
 * images of this pair list, as Cascade_Hashing_Matcher_Regions::Match builds
 * them for its whole pair list.  Later CASCADE runs whose images are a subset
 * reuse them, so a list split over ranks or batches matches exactly as the
 * whole list does; a run touching other images re-hashes for its own list. */
int sfm_match_plan_cascade_index(sfm_match_plan* plan, const int32_t* pairs,
                                 int64_t n_pairs);
/* Fetch: counts[n_pairs]; i/j/d2[total] pair-ordered, each pair's matches
 * sorted by (i, j) as openMVG IndMatch::getDeduplicated leaves them (the
 * keypoint-coordinate decorator is applied by sfm_sparse_match only). */
int sfm_match_plan_fetch(sfm_match_plan* plan, int64_t* counts,
                         uint32_t* i, uint32_t* j, int32_t* d2);
/* The same with float squared distances (any collection; a non-integer f32
 * collection has only this one). */
int sfm_match_plan_fetch_f32(sfm_match_plan* plan, int64_t* counts,
                             uint32_t* i, uint32_t* j, float* d2);
/* Order-independent digest of the last run's results (checksum of per-pair
 * checksums) computed on the device. */
int sfm_match_plan_digest(sfm_match_plan* plan, uint64_t* digest);
int sfm_match_plan_get_last_ms(sfm_match_plan* plan, double* kernel_ms,
                               int64_t* launches);
int sfm_match_plan_destroy(sfm_match_plan* plan);

/* [cpu] exhaustive pair list of openMVG exhaustivePairs(N)
 * (sparseBuilder.cpp:786): all (i, j), 0 <= i < j < N, in i-major order.
 * pairs[2 * N*(N-1)/2]. */
int sfm_exhaustive_pairs(int32_t n_img, int32_t* pairs);

/* [cpu] Deterministic synthetic RootSIFT-like descriptors for config C3:
 * n_img frames x n_kp descriptors; frames share landmark descriptors with
 * their neighbours (true correspondences) plus integer noise. */
int sfm_synth_descriptors(int32_t n_img, int32_t n_kp, uint64_t seed,
                          uint8_t* desc /* [n_img*n_kp*128] */);
/* [cpu] Deterministic gray test image, w x h bytes: 900 Gaussian blobs drawn
 * from (seed, index) on a mid-gray ground, seen rotated by angle about the
 * centre, scaled and shifted by (tx, ty), so that views of one seed share true
 * correspondences.  The generator of the golden SIFT fixtures (tests/golden,
 * oracle/vlsift_tool.c), restated. */
int sfm_synth_image(int32_t w, int32_t h, uint64_t seed, double angle, double tx, double ty, double scale,
                    uint8_t* gray /* [w*h] */);

/* ------------------------------------------------------------------------ */
/* Incremental loop: SequentialActuator (src/actuator/SequentialActuator.h)  */
/* as src/main.cpp:99-108 drives it (BASELINE.json config C5):               */
/*   init(img0, img1); bundleAdjustment();                                  */
/*   for i >= 2 { addSingleImage(img_i); bundleAdjustment(); }               */
/* LocalFrame mutual matching + 4*min filter and GlobalFrame world-point     */
/* matching + 3*min filter run on the GPU matcher (sfm_match_dense MUTUAL);  */
/* bundleAdjustment is a fresh BundleAdjuster over the whole world per call  */
/* (:226-229) on the GPU solver (sfm_ba_solve).  The OpenCV geometry          */
/* (findEssentialMat / recoverPose / solvePnPRansac) is not part of this     */
/* loop: each image carries the pose that solver would return (pose_prior)   */
/* and the inlier masks are geometric checks against the current poses (the  */
/* C++ header include/sfm/actuator.hpp documents each stand-in).  The batch  */
/* stages that estimate such poses are sfm_relpose ("Relative pose": the     */
/* first two images) and sfm_resect ("Camera resection": every later one).   */
/* ------------------------------------------------------------------------ */
typedef struct sfm_seq_image {
    int32_t n_kp;
    int32_t reserved;
    const double* kp_xy;     /* [2*n_kp] keypoint pixel coordinates           */
    const uint8_t* desc;     /* [n_kp*128] descriptors (RootSIFT uchar)       */
    double pose_prior[6];    /* Tcw as angle-axis + t (the geometric solver's
                                output; image 0's is ignored: Tcw = I)       */
} sfm_seq_image;

typedef struct sfm_seq_options {
    double fx, fy, cx, cy;   /* the one shared Camera (main.cpp:91,124)       */
    double epipolar_px;      /* essential-matrix inlier threshold, px (4.0)   */
    double pnp_reproj_px;    /* solvePnPRansac reprojectionError (8.0, :179)  */
    double max_depth;        /* recoverPose distanceThresh (100)              */
    int64_t min_pnp_inliers; /* drop the image below this (30, :191)          */
    int32_t fixed_writeback; /* 0: Image::setIntrinsic ZYX-Euler quirk (the
                                reference); 1: store the angle-axis          */
    int32_t reserved;
    sfm_ba_options ba;       /* BundleAdjuster() solver options               */
} sfm_seq_options;

/* What one init / addSingleImage (+ the following bundleAdjustment) did. */
typedef struct sfm_seq_step {
    int32_t image;              /* sequence index of the new image           */
    int32_t kept;               /* 0: dropped (< min_pnp_inliers)            */
    int64_t local_raw, local_kept;     /* LocalFrame matches before / after
                                          the 4*min filter                  */
    int64_t global_raw, global_kept;   /* GlobalFrame, 3*min filter          */
    int64_t pnp_inliers, epipolar_inliers;
    int64_t new_points, extended_obs;  /* savePointCloudToWorld             */
    int64_t world_points, world_observations;
    sfm_ba_summary ba;          /* last bundleAdjustment of this step        */
    int32_t ba_rc;              /* its return code (1: not run yet)          */
    int32_t reserved;
    int64_t ba_images, ba_points, ba_observations;   /* its problem size    */
    double seconds_local_match, seconds_global_match, seconds_geometry, seconds_ba;
} sfm_seq_step;

typedef struct sfm_seq sfm_seq;
/* [cpu] SequentialActuator defaults + BundleAdjuster() options. */
void sfm_seq_default_options(sfm_seq_options* opts);
int sfm_seq_create(sfm_ctx* ctx, const sfm_seq_options* opts, sfm_seq** out);
int sfm_seq_init(sfm_seq* seq, const sfm_seq_image* img0, const sfm_seq_image* img1);
/* *kept = 0 when the image was dropped (fewer than min_pnp_inliers). */
int sfm_seq_add_image(sfm_seq* seq, const sfm_seq_image* img, int32_t* kept);
int sfm_seq_bundle_adjust(sfm_seq* seq, sfm_ba_summary* summary);
int sfm_seq_last_step(sfm_seq* seq, sfm_seq_step* step);
/* The last step's filtered matches: which 0 = LocalFrame (query = image1
 * keypoint, train = image2 keypoint), 1 = GlobalFrame (query = world point in
 * index order, train = image keypoint).  dist = sqrt of the exact L2^2. */
int sfm_seq_matches(sfm_seq* seq, int32_t which, int32_t* query, int32_t* train,
                    float* dist, int64_t cap, int64_t* n);
/* World state: points in index order (X[3*n]), the observation count of
 * each (n_obs[n]), every image's pose in sequence order (poses[6*n_img]) and
 * the shared camera's {fx, fy, cx, cy}.  NULL arrays: sizes only. */
int sfm_seq_world(sfm_seq* seq, double* X, int64_t* n_obs, int64_t cap_pts, int64_t* n_pts,
                  double* poses, int32_t cap_img, int32_t* n_img, double* intr4);
/* Every world point's observations, points in index order (counts from
 * sfm_seq_world's n_obs): the observing image's sequence index and the pixel. */
int sfm_seq_observations(sfm_seq* seq, int32_t* img, double* uv, int64_t cap, int64_t* n);
int sfm_seq_destroy(sfm_seq* seq);

/* [cpu] Synthetic closed-orbit image sequence for C5: cameras on a circle of
 * radius 10 around a cube of landmarks (side 4), looking at its centre, all
 * with the reference intrinsics (fx = fy = 2905.88, cx 1416, cy 1064).  Each
 * landmark faces a direction and is seen from an arc of consecutive images
 * (tracks of ~track_mean images), detected with detect_prob; its observed
 * descriptor is a RootSIFT-like base with desc_noise_dims entries moved by up
 * to +-desc_noise_amp.  n_clutter unmatched keypoints per image.  Keypoint
 * order is shuffled per image.  pose_prior = ground-truth Tcw relative to
 * image 0 (the reconstruction's world frame) + N(0, prior_rot^2) rad /
 * N(0, prior_t^2) noise; image 0's is exactly zero. */
typedef struct sfm_synth_orbit_config {
    int32_t n_img, n_clutter;
    int64_t n_landmarks;
    double track_mean, detect_prob, noise_px;
    int32_t desc_noise_dims, desc_noise_amp;
    double prior_rot, prior_t;
    uint64_t seed;
} sfm_synth_orbit_config;
/* Two calls: NULL arrays return *n_kp only.  landmark[n_kp] (optional):
 * ground-truth landmark of each keypoint or -1 for clutter; gt_X (optional,
 * [3*n_landmarks]) landmark positions in the image-0 frame. */
int sfm_synth_orbit_image(const sfm_synth_orbit_config* cfg, int32_t img, int32_t* n_kp,
                          double* kp_xy, uint8_t* desc, double* pose_prior,
                          int64_t* landmark, double* gt_X);

/* ------------------------------------------------------------------------ */
/* File-staged sparseBuilder flow.                   */
/* The reference's matchPair()/match() (sparseBuilder.cpp:758-1023) talk to  */
/* each other through files in <base>/output/matches written by OpenMVG's    */
/* Load/Save (cereal).  These functions read and write the same layouts      */
/* natively (restated from OpenMVG's published code; OpenMVG is un-vendored, */
/* so byte parity is unpinned — DESIGN.md §3).  Pass NULL output arrays to   */
/* query sizes first.                                                        */
/* ------------------------------------------------------------------------ */
typedef struct sfm_mvg_view {  /* openMVG::sfm::View                         */
    uint32_t id_view, id_intrinsic, id_pose, width, height;
    char img_path[500];        /* View::s_Img_path = local_path/filename      */
} sfm_mvg_view;

/* [cpu] VIEWS of an sfm_data.json (Load(sfm_data, ..., VIEWS), :773, :835),
 * sorted by id_view. */
int sfm_mvg_load_views(const char* sfm_data_json, sfm_mvg_view* views,
                       int32_t cap, int32_t* n_views);
/* [cpu] image_describer.json names 128-D uint8 SIFT_Regions (:851-856);
 * other region types return SFM_ERR_UNSUPPORTED. */
int sfm_mvg_check_describer(const char* image_describer_json);
/* [cpu] <stem>.desc: uint64 count, count x 128 uint8 (saveDescsToBinFile). */
int sfm_mvg_read_desc(const char* path, uint8_t* desc, int64_t cap_rows, int64_t* n_rows);
int sfm_mvg_write_desc(const char* path, const uint8_t* desc, int64_t n_rows);
/* [cpu] <stem>.feat: text "x y scale orientation" per keypoint (SIOPointFeature). */
int sfm_mvg_read_feat(const char* path, float* xyso /* [4*n] */, int64_t cap_rows, int64_t* n_rows);
/* nine significant digits per number, so that reading gives the same floats back */
int sfm_mvg_write_feat(const char* path, const float* xyso /* [4*n] */, int64_t n_rows);
/* [cpu] pairs.bin (text despite its name): loadPairs(N, ...) / savePairs
 * (:801, :948): lines "I J1 J2 ...", stored as sorted unique (min, max). */
int sfm_mvg_load_pairs(const char* path, int32_t n_views, int32_t* pairs, int64_t cap,
                       int64_t* n_pairs);
int sfm_mvg_save_pairs(const char* path, const int32_t* pairs, int64_t n_pairs);
/* [cpu] PairWiseMatches Save/Load (:986, :896): ".bin" = cereal
 * PortableBinary (uint8 1; uint64 #pairs; per pair uint32 I, J, uint64 n,
 * n x (uint32 i, j)), ".txt" = "I J\nn\ni j\n...".  pairs strictly increasing. */
int sfm_mvg_save_matches(const char* path, const int32_t* pairs, int64_t n_pairs,
                         const int64_t* counts, const uint32_t* i, const uint32_t* j);
int sfm_mvg_load_matches(const char* path, int32_t* pairs, int64_t* counts,
                         uint32_t* i, uint32_t* j, int64_t cap_pairs, int64_t cap_matches,
                         int64_t* n_pairs, int64_t* n_matches);

/* [cpu] sparseBuilder::matchPair(): <matches_dir>/pairs.bin =
 * exhaustivePairs(#views of sfm_data.json). */
int sfm_sparse_match_pair(const char* matches_dir);

typedef struct sfm_sparse_match_opts {
    int32_t mode;      /* SFM_MATCH_CASCADE = "AUTO", the reference's default
                          (:814, :911-914); SFM_MATCH_RATIO = "BRUTEFORCEL2"
                          (:919-921); NULL opts select CASCADE             */
    float ratio;       /* fDistRatio 0.8f (:812)                              */
    int32_t force;     /* 0: reload an existing matches.putative.bin (:890)   */
    int32_t dedup_xy;  /* 1: drop matches whose keypoint coordinates repeat
                          (IndMatchDecorator, needs <stem>.feat)             */
    int32_t reserved[2];
} sfm_sparse_match_opts;
typedef struct sfm_sparse_match_stats {
    int64_t n_views, n_pairs_in, n_pairs_out, n_matches;
    int32_t reloaded, reserved;
} sfm_sparse_match_stats;
/* sparseBuilder::match(), file-staged: sfm_data.json + image_describer.json
 * + <stem>.desc/.feat + pairs.bin -> GPU matcher ->
 * matches.putative.bin (non-empty pairs) + preemptive_pairs.txt.
 * pairs.bin must exist (the reference's loadPairs fails without it, :957-960:
 * SFM_ERR_INVALID_ARG).  opts NULL = {CASCADE ("AUTO"), 0.8f, 0, 1}.
 * dedup_xy keeps the survivors in the order OpenMVG's
 * IndMatchDecorator::getDeduplicated leaves them (std::set over its
 * coordinate comparator, inserted in (i, j) order). */
int sfm_sparse_match(sfm_ctx* ctx, const char* matches_dir, const sfm_sparse_match_opts* opts,
                     sfm_sparse_match_stats* stats);

/* ------------------------------------------------------------------------ */
/* Geometric filter                                  */
/* sparseBuilder::filter() (sparseBuilder.cpp:1025-1280) runs                */
/* GeometricFilter_FMatrix_AC(4.0, 2048) (:1179-1186) over every putative    */
/* pair: OpenMVG's a-contrario RANSAC (ACRANSAC) with the 7-point            */
/* fundamental-matrix solver, keeping a pair iff it has > 2.5 * 7 inliers.   */
/* Restated from OpenMVG's published code (un-vendored: parity unpinned,     */
/* DESIGN.md §3); the GPU runs one workgroup per pair.                       */
/* ------------------------------------------------------------------------ */
typedef struct sfm_fmatrix_opts {
    double precision;         /* 4.0 px: upper bound of the a-contrario threshold */
    int32_t max_iterations;   /* 2048 (imax_iteration, :1040)                     */
    int32_t reserved;
} sfm_fmatrix_opts;
typedef struct sfm_fmatrix_result {
    double F[9];          /* row-major, pixels: x_J' F x_I = 0 (when n_inliers > 0)  */
    double error_max;     /* a-contrario threshold in px (ACRANSAC .first)          */
    double min_nfa;       /* log10 NFA of the best model (ACRANSAC .second)         */
    int32_t n_inliers;    /* > 17 when the pair is kept, else 0                     */
    int32_t iterations;   /* RANSAC iterations run                                  */
} sfm_fmatrix_result;
/* n_pairs independent pairs.  Pair q's putative correspondences are
 * k = off[q] .. off[q+1]-1 with xy[4k..4k+3] = (x_I, y_I, x_J, y_J) in pixels
 * (MatchesPairToMat order = the putative IndMatch order); wh[4q..4q+3] =
 * (width_I, height_I, width_J, height_J).  inliers[off[q] + t],
 * t < results[q].n_inliers: the kept correspondences (indices into the pair's
 * list) in OpenMVG's vec_inliers order (ascending residual).  opts NULL =
 * {4.0, 2048}.  Pairs of any size (sort buffers move from LDS to global
 * memory above 8192 correspondences); a pair whose RANSAC would draw more than
 * 2^18 random numbers (2048 iterations draw about 15,000) returns
 * SFM_ERR_UNSUPPORTED. */
int sfm_fmatrix_ac(sfm_ctx* ctx, int64_t n_pairs, const int64_t* off, const double* xy,
                   const int32_t* wh, const sfm_fmatrix_opts* opts,
                   sfm_fmatrix_result* results, int32_t* inliers);

/* Device time (HIP events on the context's stream) of the kernel(s) of the
 * context's last sfm_fmatrix_ac, sfm_triangulate, sfm_tracks_build (also
 * through sfm_sparse_tracks), sfm_resect or sfm_relpose call, without its host
 * normalisation, uploads and downloads (measurement; no reference counterpart).  Only a
 * context created with SFM_CTX_TIME_KERNELS times it; -1 otherwise. */
int sfm_ctx_last_kernel_ms(sfm_ctx* ctx, double* ms);

/* sparseBuilder::filter(), file-staged: sfm_data.json (view sizes) +
 * <stem>.feat + matches.putative.bin -> sfm_fmatrix_ac ->
 * matches.f.bin (kept pairs, each pair's IndMatches in vec_inliers order).
 * opts NULL = {4.0, 2048}. */
typedef struct sfm_sparse_filter_stats {
    int64_t n_pairs_in, n_pairs_out, n_matches_in, n_matches_out;
} sfm_sparse_filter_stats;
int sfm_sparse_filter(sfm_ctx* ctx, const char* matches_dir, const sfm_fmatrix_opts* opts,
                      sfm_sparse_filter_stats* stats);

/* ------------------------------------------------------------------------ */
/* Post-BA outlier rejection ("wash")                                        */
/* The step BundleAdjuster::operator() left as a hook between the solve and  */
/* updateWorld() (src/adjuster/BundleAdjuster.h:179-184, washPoint()), and    */
/* the filter OpenMVG's engine runs after every BA (badTrackRejector(4.0):   */
/* RemoveOutliers_PixelResidualError(4.0 px, min track length 2), then       */
/* RemoveOutliers_AngleError(2.0 deg)); restated, parity unpinned            */
/* (DESIGN.md §3).                                                           */
/*                                                                          */
/* Observation o of point p in image i: P = R(w_i) X_p + t_i, r = the        */
/* unweighted residual of the problem's camera_model (what the solver        */
/* squares before the loss).  It is rejected by the first rule that applies: */
/*   depth     r is not finite, or cheirality != 0 and the point is not in   */
/*             front of the camera (P[2] > 0; SFM_CAM_SNAVELY looks down -z: */
/*             P[2] < 0)                                                     */
/*   residual  max_residual_px > 0 and |r| > max_residual_px                 */
/* Point p: over its surviving observations the rays d = R_i' P (camera      */
/* centre to point, world axes); max_angle_deg = the largest angle between   */
/* two of them, atan2(|a x b|, a.b) in degrees (0 with fewer than two; two   */
/* observations in one image give 0).  OpenMVG takes the back-projected      */
/* pixel bearing instead, which differs by the surviving residual only.  The */
/* point is removed by the first rule that applies:                          */
/*   short     survivors < min_track_len                                     */
/*   angle     min_angle_deg > 0 and max_angle_deg < min_angle_deg           */
/* and every observation of a removed point gets keep_obs = 0.               */
/* ------------------------------------------------------------------------ */
typedef struct sfm_ba_wash_opts {
    double max_residual_px;   /* 4.0; <= 0: no residual rule                   */
    double min_angle_deg;     /* 2.0; <= 0: no angle rule                      */
    int32_t min_track_len;    /* 2 (>= 1)                                      */
    int32_t cheirality;       /* 1                                             */
} sfm_ba_wash_opts;
typedef struct sfm_ba_wash_stats {
    int64_t n_obs_depth, n_obs_residual;   /* rejected observations, by rule   */
    int64_t n_pt_short, n_pt_angle;        /* removed points, by rule          */
    int64_t n_obs_kept, n_pt_kept;
} sfm_ba_wash_stats;
/* [cpu] {4.0, 2.0, 2, 1}; NULL opts below select them. */
void sfm_ba_wash_default_options(sfm_ba_wash_opts* opts);

/* One-shot: uploads the problem and the parameters, evaluates, downloads.
 * Outputs are in the problem's own observation / point order; any of them may
 * be NULL.  It does not shard: on a world_size > 1 context every rank
 * evaluates the whole problem.  Argument checks as sfm_ba_plan_create's, and
 * min_track_len >= 1 (SFM_ERR_INVALID_ARG). */
int sfm_ba_wash(sfm_ctx* ctx, const sfm_ba_problem* prob, const double* extr, const double* intr,
                const double* X, const sfm_ba_wash_opts* opts, double* residual /* [2*n_obs] */,
                double* max_angle_deg /* [n_pt] */, uint8_t* keep_obs /* [n_obs] */,
                uint8_t* keep_pt /* [n_pt] */, sfm_ba_wash_stats* stats);

/* Resident: at the plan's current parameters (what sfm_ba_plan_download
 * returns; before the first run, the parameters the plan was created with) on
 * the observations already in HBM: nothing observation-sized is uploaded.
 * The same outputs, bit for bit, as sfm_ba_wash at those parameters.  What it
 * needs beyond the plan's arrays (the map from the plan's sorted layout to
 * the problem's order, scratch) is built by the first call and kept.  A plan
 * of a world_size > 1 context returns SFM_ERR_UNSUPPORTED (a shard holds only
 * its own points). */
int sfm_ba_plan_wash(sfm_ba_plan* plan, const sfm_ba_wash_opts* opts, double* residual,
                     double* max_angle_deg, uint8_t* keep_obs, uint8_t* keep_pt,
                     sfm_ba_wash_stats* stats);
/* Device time (HIP events) of the two kernels of the plan's last
 * sfm_ba_plan_wash: the observation pass and the point pass.  Only a plan of
 * a context created with SFM_CTX_TIME_KERNELS times them; -1 otherwise. */
int sfm_ba_plan_wash_last_ms(sfm_ba_plan* plan, double* obs_ms, double* point_ms);

/* [cpu] The washed problem: the kept points in their old order, each with its
 * kept observations in their old order; images, intrinsics, const_img and the
 * model are untouched (the planner takes unobserved images).  pt_map[k] = the
 * old index of new point k.  The output arrays are sized from the wash's
 * stats: pt_offsets[n_pt_kept + 1], obs_img[n_obs_kept], obs_uv[2*n_obs_kept],
 * X_out[3*n_pt_kept], pt_map[n_pt_kept]; any may be NULL.  A kept observation
 * of a removed point is SFM_ERR_INVALID_ARG. */
int sfm_ba_wash_apply(const sfm_ba_problem* prob, const double* X, const uint8_t* keep_obs,
                      const uint8_t* keep_pt, int64_t* pt_offsets, int32_t* obs_img, double* obs_uv,
                      double* X_out, int64_t* pt_map);

/* ------------------------------------------------------------------------ */
/* Track triangulation                                                       */
/* Points from known poses and tracks: OpenMVG's                             */
/* ComputeStructureFromKnownPoses, and what its incremental engine does for  */
/* new tracks after each resection (the reference triangulates two views at  */
/* SequentialActuator.h:206-223).  The N-view solve is OpenMVG's             */
/* TriangulateNViewAlgebraic; restated from its published code, parity       */
/* unpinned.  ROBUST deliberately replaces OpenMVG's random   */
/* minimal samples by an exhaustive (or, past max_hypotheses, evenly spread) */
/* set of view pairs: every decision is a deterministic function of the      */
/* input.                                                                    */
/*                                                                          */
/* The input is a sfm_ba_problem (const_img and huber_a are ignored) and the */
/* cameras.  Per point, over its observations in order:                      */
/*   bearing   PINHOLE b = ((u-cx)/fx, (v-cy)/fy, 1); RADIAL3 p_d =          */
/*             ((u-ppx)/f, (v-ppy)/f), undistorted by exactly 20 iterations  */
/*             p_u <- p_d / c(|p_u|^2) from p_u = p_d, b = (p_u, 1); SNAVELY */
/*             p_d = (u/f, v/f), the same iteration with d(), b = (p_u, -1). */
/*             b is normalised; an observation whose b is not finite is bad: */
/*             it takes no part in any solve (n_obs_bad).                    */
/*   solve     over a set of observations: M = sum C'C, C = (I - b b')[R|t], */
/*             summed in observation order; v = the eigenvector of M's       */
/*             smallest eigenvalue (cyclic Jacobi, at most 30 sweeps),       */
/*             X = v[0..2] / v[3]; INFINITE unless |v[3]| > 1e-12 and X is   */
/*             finite.                                                       */
/*   judge     an observation at X, by sfm_ba_wash's rules: depth (residual  */
/*             not finite, or cheirality and not in front), else residual    */
/*             (max_residual_px > 0 and |r| > max_residual_px).              */
/*   LINEAR    one solve over every good observation; keep_obs = those that  */
/*             pass the judgement at X (no refit).                           */
/*   ROBUST    hypotheses = the pairs (a, b), a < b, of good observations of */
/*             different images, in lexicographic order; when there are more */
/*             than max_hypotheses, pair floor(h * npairs / max_hypotheses)  */
/*             for h = 0 .. max_hypotheses-1.  Each is solved from its two   */
/*             views and judged on every good observation; the best has the  */
/*             most inliers, then the smallest sum of squared inlier         */
/*             residuals, then the lowest h (an INFINITE hypothesis has no   */
/*             inliers).  One solve over the winner's inliers, and one       */
/*             judgement of every observation at that X: keep_obs.           */
/* Point status, the first that applies:                                     */
/*   SHORT     fewer than two good observations, no hypothesis, a ROBUST     */
/*             winner with fewer than two inliers (nothing to solve from);   */
/*   INFINITE  the final solve;                                              */
/*   SHORT     fewer than min_track_len kept observations;                   */
/*   ANGLE     min_angle_deg > 0 and the largest angle between two kept      */
/*             observations' measured rays R' b, atan2(|a x b|, a.b), is     */
/*             below it (exactly 0 for two observations of one image).       */
/* A point that is not OK gets X = NaN and keep_obs = 0 throughout.          */
/* residual is the residual at the final X of the solve (also when the point */
/* was then removed as SHORT or ANGLE); NaN where there is no such X and at  */
/* bad observations.  n_obs_depth / n_obs_residual count the final           */
/* judgement's rejections.                                                   */
/* ------------------------------------------------------------------------ */
#define SFM_TRI_LINEAR 0   /* every observation, one N-view algebraic solve      */
#define SFM_TRI_ROBUST 1   /* two-view hypotheses, consensus, N-view refit        */
#define SFM_TRI_OK       0
#define SFM_TRI_SHORT    1
#define SFM_TRI_ANGLE    2
#define SFM_TRI_INFINITE 3
typedef struct sfm_tri_opts {
    int32_t method;           /* SFM_TRI_ROBUST                                   */
    int32_t max_hypotheses;   /* 64 (>= 1): ROBUST hypotheses per point           */
    double  max_residual_px;  /* 4.0; <= 0: no residual rule                      */
    double  min_angle_deg;    /* 2.0; <= 0: no angle rule                         */
    int32_t min_track_len;    /* 2 (>= 2)                                         */
    int32_t cheirality;       /* 1                                                */
} sfm_tri_opts;
typedef struct sfm_tri_stats {
    int64_t n_pt_ok, n_pt_short, n_pt_angle, n_pt_infinite;
    int64_t n_obs_kept, n_obs_bad, n_obs_depth, n_obs_residual;
} sfm_tri_stats;
/* [cpu] {ROBUST, 64, 4.0, 2.0, 2, 1}; NULL opts below select them. */
void sfm_tri_default_options(sfm_tri_opts* opts);
/* One-shot: uploads the problem and the cameras, triangulates every point,
 * downloads.  Outputs are in the problem's own order; any may be NULL.
 * Argument checks as sfm_ba_wash's, method, min_track_len >= 2 and
 * max_hypotheses >= 1 (SFM_ERR_INVALID_ARG).  It does not shard: on a
 * world_size > 1 context every rank triangulates the whole problem.  A
 * context created with SFM_CTX_TIME_KERNELS reports the kernels' device time
 * through sfm_ctx_last_kernel_ms. */
int sfm_triangulate(sfm_ctx* ctx, const sfm_ba_problem* prob, const double* extr, const double* intr,
                    const sfm_tri_opts* opts, double* X /* [3*n_pt] */, uint8_t* status /* [n_pt] */,
                    uint8_t* keep_obs /* [n_obs] */, double* residual /* [2*n_obs] */, sfm_tri_stats* stats);
/* [cpu] The same on the host, a serial loop over the same per-point code
 * (results agree with the device's to rounding, not bit for bit). */
int sfm_triangulate_host(const sfm_ba_problem* prob, const double* extr, const double* intr,
                         const sfm_tri_opts* opts, double* X, uint8_t* status, uint8_t* keep_obs,
                         double* residual, sfm_tri_stats* stats);

/* ------------------------------------------------------------------------ */
/* Track building                                                            */
/* Pairwise feature matches (matches.f.bin, what sfm_sparse_filter writes)   */
/* into tracks: the first step of OpenMVG's reconstruction engines, which    */
/* reconstruction() runs on matches.f.bin (sparseBuilder.cpp:1435,           */
/* :1474-1508): tracks::TracksBuilder Build + Filter + ExportToSTL.          */
/* Restated from its published code, parity unpinned.         */
/*                                                                          */
/* A node is (image, feature); only nodes named by a match exist.  An edge   */
/* is one match (I, i) - (J, j); a component is a connected component.  A    */
/* component is removed by the first rule that applies:                      */
/*   conflict  two of its nodes are different features of one image;         */
/*   short     it has fewer than min_track_len nodes.                        */
/* What remains are the tracks, in a canonical order (OpenMVG's track ids    */
/* are union-find roots and depend on its implementation): tracks by their   */
/* smallest node (image, then feature), observations inside a track by       */
/* image.  The set of tracks and each track's map<image, feature> order are  */
/* OpenMVG's STLMAPTracks.  The tracks are a function of the set of edges:   */
/* pair order, match order, repeated matches and a pair given as (J, I)      */
/* change nothing (of the stats, n_edges alone counts the matches as given,  */
/* repeats included).                                                        */
/* ------------------------------------------------------------------------ */
typedef struct sfm_tracks sfm_tracks;
typedef struct sfm_tracks_opts {
    int32_t min_track_len;    /* 2 (>= 2)                                         */
    int32_t reserved[3];
} sfm_tracks_opts;
typedef struct sfm_tracks_stats {
    int64_t n_nodes, n_edges, n_components;   /* n_edges: the matches given        */
    int64_t n_conflict, n_short;              /* removed components, by rule       */
    int64_t n_tracks, n_obs, max_track_len;   /* what is kept                      */
} sfm_tracks_stats;
/* [cpu] {2}; NULL opts below select it. */
void sfm_tracks_default_options(sfm_tracks_opts* opts);
/* Image I has features feat_off[I] .. feat_off[I+1]-1 as dense node ids
 * (feat_off[0] >= 0, non-decreasing; an image may have none).  pairs, counts,
 * i, j: sfm_mvg_save_matches' layout (pair q = images pairs[2q], pairs[2q+1],
 * its counts[q] matches consecutive in i / j).  xy (optional): a position per
 * node id, which sfm_tracks_fetch gathers into obs_uv.  Every argument check
 * runs on the host before any device call: I == J, an image outside
 * [0, n_img), a feature index at or past its image's count, a decreasing
 * feat_off, min_track_len < 2: SFM_ERR_INVALID_ARG; feat_off[n_img] or the
 * number of matches above 2^31 - 1: SFM_ERR_UNSUPPORTED.  No matches give zero
 * tracks.  It does not shard.  A context created with SFM_CTX_TIME_KERNELS
 * reports the kernels' device time through sfm_ctx_last_kernel_ms. */
int sfm_tracks_build(sfm_ctx* ctx, int32_t n_img, const int64_t* feat_off /* [n_img+1] */,
                     int64_t n_pairs, const int32_t* pairs /* [2*n_pairs] */, const int64_t* counts,
                     const uint32_t* i, const uint32_t* j, const double* xy /* [2*feat_off[n_img]] or NULL */,
                     const sfm_tracks_opts* opts, sfm_tracks** out);
/* [cpu] The same from a serial union-find on the host: the same outputs bit
 * for bit (everything is integral, obs_uv is a gather). */
int sfm_tracks_build_host(int32_t n_img, const int64_t* feat_off, int64_t n_pairs, const int32_t* pairs,
                          const int64_t* counts, const uint32_t* i, const uint32_t* j, const double* xy,
                          const sfm_tracks_opts* opts, sfm_tracks** out);
/* [cpu] */
int sfm_tracks_get_stats(sfm_tracks* t, sfm_tracks_stats* stats);
/* [cpu] The tracks as a sfm_ba_problem takes them: pt_offsets[n_tracks+1]
 * (pt_offsets = {0} without tracks), obs_img[n_obs], obs_feat[n_obs] (the
 * feature's index in its image), obs_uv[2*n_obs]; any may be NULL.  obs_uv of
 * a handle built without xy is SFM_ERR_INVALID_ARG. */
int sfm_tracks_fetch(sfm_tracks* t, int64_t* pt_offsets, int32_t* obs_img, uint32_t* obs_feat,
                     double* obs_uv);
/* [cpu] */
int sfm_tracks_destroy(sfm_tracks* t);
/* File-staged: the views of <matches_dir>/sfm_data.json (image I = the I-th
 * view by id_view), every <stem>.feat (the feature counts, and x y as xy) and
 * <matches_dir>/<matches_file> (NULL: matches.f.bin), then sfm_tracks_build.
 * A match naming a view that sfm_data.json lacks is SFM_ERR_INVALID_ARG. */
int sfm_sparse_tracks(sfm_ctx* ctx, const char* matches_dir, const char* matches_file,
                      const sfm_tracks_opts* opts, sfm_tracks** out);

/* ------------------------------------------------------------------------ */
/* Camera resection                                                          */
/* The pose of an image from 2D-3D correspondences: what OpenMVG's           */
/* incremental engine (reconstruction() with engine_name "INCREMENTAL",      */
/* sparseBuilder.cpp:1289,1477) does for every image it adds:                */
/* SfM_Localizer::Localize (AC-RANSAC over a P3P solver, 4096 iterations, no */
/* upper threshold) and RefinePose on the inliers.  Restated from its        */
/* published code, parity unpinned.  n_img independent        */
/* problems; the GPU runs one workgroup per image.                           */
/*                                                                          */
/* Problem q: correspondences k = off[q] .. off[q+1]-1 (n of them), world    */
/* point X[3k..], pixel uv[2k..], intrinsics block intr + iw * img_intr[q]   */
/* (iw = sfm_ba_intr_width(camera_model)), image size wh[2q..] = (w, h).     */
/*   bearing   of a pixel: sfm_triangulate's.  A correspondence whose        */
/*             bearing is not finite never enters a sample and has error     */
/*             +inf.  The others, in order, are the list samples draw from.  */
/*   P3P       3 correspondences -> at most 4 models (R, t), P = R X + t:    */
/*             Grunert's quartic in the ratio of two distances, its real     */
/*             roots by Ferrari's resolvent and 2 Newton steps, the three    */
/*             distances polished by 2 Newton steps on the cosine laws and   */
/*             kept when all are positive, R and t by aligning the two       */
/*             triangles' frames.  Only + - * / and sqrt.  0 models for a    */
/*             collinear or repeated sample.                                 */
/*   error     of a correspondence under a model: |r|^2 in px^2, r the       */
/*             camera model's residual at P; +inf when r is not finite or P  */
/*             is not in front (P2 > 0; P2 < 0 for SNAVELY).                 */
/*   AC-RANSAC OpenMVG's ACRANSAC as sfm_fmatrix_ac restates it: the         */
/*             mt19937(default_seed) stream from position 0 per problem, the */
/*             same uniform_int restatement, two sampling modes, 10 %        */
/*             iteration reserve, focused resampling and tie rules.  A model */
/*             counts as found with more than 2.5 * 3 errors under the       */
/*             bound.  NFA(k) = loge0 + logalpha (k-3) + logcombi(k, n) +    */
/*             logcombi(3, k), k = 4 .. m, over the m errors under the bound */
/*             in ascending (error, index) order, logalpha = logalpha0 +     */
/*             log10(e_k + FLT_EPSILON), logalpha0 = log10(pi / (w h)),      */
/*             loge0 = log10(4 (n - 3)); the two logcombi tables are rounded */
/*             to float, as OpenMVG's.  The bound is precision^2;            */
/*             precision <= 0 or +inf: none (every finite error).            */
/*             Kept iff min_nfa < 0 and n_inliers > 7.                       */
/*   refit     on a kept problem's inliers, from the RANSAC model: up to     */
/*             refine_iterations Gauss-Newton steps on (R <- exp[d]x R,      */
/*             t += d_t) with the camera model's residual and its analytic   */
/*             Jacobian, no loss; an inlier behind the camera (or with a     */
/*             residual that is not finite) at an iterate is skipped; stops  */
/*             once |d|^2 < 1e-24.  A singular 6x6 system (or a rotation     */
/*             step above 1 rad) leaves the RANSAC model in place.  The      */
/*             inlier set is not re-evaluated after the refit.               */
/* status: SFM_RESECT_FEW (n <= 3, or fewer than 4 finite bearings:          */
/* everything 0), SFM_RESECT_NO_MODEL (not kept: n_inliers 0, both poses and */
/* error_max 0, min_nfa the best seen, +inf when none), SFM_RESECT_OK.       */
/* Two device runs give the same bits.  Host and device run the same         */
/* statements and differ by rounding only.                                   */
/* ------------------------------------------------------------------------ */
#define SFM_RESECT_OK       0
#define SFM_RESECT_FEW      1
#define SFM_RESECT_NO_MODEL 2
typedef struct sfm_resect_opts {
    double  precision;          /* px; <= 0 or +inf: no upper bound (the engine) */
    int32_t max_iterations;     /* 4096 (>= 1)                                    */
    int32_t refine_iterations;  /* 10 (>= 0)                                      */
} sfm_resect_opts;
typedef struct sfm_resect_result {
    double  pose[6];        /* refined: angle-axis, then t (the extrinsics layout) */
    double  pose_model[6];  /* the RANSAC model before the refit                   */
    double  error_max;      /* px: square root of the a-contrario threshold        */
    double  min_nfa;        /* log10 NFA of the best model                         */
    int32_t n_inliers;
    int32_t iterations;     /* RANSAC iterations run                               */
    int32_t status;         /* SFM_RESECT_*                                        */
    int32_t reserved;
} sfm_resect_result;
/* [cpu] {0 (no bound), 4096, 10}; NULL opts below select them. */
void sfm_resect_default_options(sfm_resect_opts* opts);
/* inliers[off[q] + t], t < results[q].n_inliers: the inliers (indices into
 * the problem's list) in ascending (error, index) order at the RANSAC model;
 * the rest of inliers[] is left alone.  Every argument check runs on the host
 * before any device call: a null pointer, negative counts, off[0] != 0 or off
 * not monotone, an unknown camera_model, img_intr outside [0, n_intr), a
 * non-positive image size, max_iterations < 1, refine_iterations < 0 or a NaN
 * precision: SFM_ERR_INVALID_ARG; n_img or off[n_img] >= 2^31, or a problem
 * drawing more than 2^18 random numbers: SFM_ERR_UNSUPPORTED.  Problems of
 * any size (the sort moves from LDS to global memory above 8192
 * correspondences).  It does not shard.  A context created with
 * SFM_CTX_TIME_KERNELS reports the kernel's device time through
 * sfm_ctx_last_kernel_ms. */
int sfm_resect(sfm_ctx* ctx, int32_t camera_model, int64_t n_img, const int64_t* off /* [n_img+1] */,
               const double* X /* [3*n] */, const double* uv /* [2*n] */, const int32_t* img_intr /* [n_img] */,
               const double* intr /* [iw*n_intr] */, int32_t n_intr, const int32_t* wh /* [2*n_img] */,
               const sfm_resect_opts* opts, sfm_resect_result* results /* [n_img] */, int32_t* inliers /* [n] */);
/* [cpu] The same on the host, a serial loop over the same statements. */
int sfm_resect_host(int32_t camera_model, int64_t n_img, const int64_t* off, const double* X, const double* uv,
                    const int32_t* img_intr, const double* intr, int32_t n_intr, const int32_t* wh,
                    const sfm_resect_opts* opts, sfm_resect_result* results, int32_t* inliers);
/* [cpu] The minimal solver alone: unit bearings b[3i..] and world points
 * X[3i..], i < 3; *n models, model m = Rt[m][0..8] (R row-major), Rt[m][9..11] (t). */
int sfm_resect_p3p(const double b[9], const double X[9], double Rt[4][12], int32_t* n);
/* [cpu] The 2D-3D correspondences of the n_images images listed in images[]
 * (each in [0, prob->n_img)): the observations of image images[q] whose point
 * p has pt_ok[p] != 0, in the problem's order, as off[n_images+1] and, unless
 * NULL, X3[3k..] = X[3p..] and uv[2k..].  With X3 and uv NULL it returns the
 * counts only (over every image: which images can be resected next). */
int sfm_resect_gather(const sfm_ba_problem* prob, const double* X, const uint8_t* pt_ok, const int32_t* images,
                      int32_t n_images, int64_t* off, double* X3, double* uv);

/* ------------------------------------------------------------------------ */
/* Relative pose                                                             */
/* The relative pose of an image pair from its 2D-2D matches: what OpenMVG's */
/* incremental engine (reconstruction() with no initial pair given,          */
/* sparseBuilder.cpp:1289,1302,1493) runs on every matched pair to choose    */
/* the pair it starts from, and again on the winner: robustRelativePose      */
/* (AC-RANSAC over the five-point essential-matrix solver, 4096 iterations)  */
/* and the cheirality selection among the four motions.  Restated from its   */
/* published code, parity unpinned.  n_pairs independent      */
/* problems; the GPU runs one workgroup per pair.                            */
/*                                                                          */
/* Problem q: correspondences k = off[q] .. off[q+1]-1 (n of them), pixel    */
/* xy[4k..] = (x_I, y_I, x_J, y_J), intrinsics blocks intr + iw *            */
/* pair_intr[2q] (image I) and intr + iw * pair_intr[2q+1] (image J), iw =   */
/* sfm_ba_intr_width(camera_model), image sizes wh[4q..] = (w_I, h_I, w_J,   */
/* h_J): the layouts of sfm_fmatrix_ac.                                      */
/*   bearing   of a pixel: sfm_triangulate's.  A correspondence with a       */
/*             bearing that is not finite on either side never enters a      */
/*             sample and has error +inf.  The others, in order, are the     */
/*             list samples draw from.                                       */
/*   5-point   5 bearing pairs -> at most 10 matrices E with b_J' E b_I = 0, */
/*             Nister's formulation with these choices.  The 5x9 epipolar    */
/*             system in E's row-major entries is brought to reduced row     */
/*             echelon form by Gauss-Jordan elimination with complete        */
/*             pivoting: each step takes the largest |entry| over the rows   */
/*             not yet used and the columns not yet used, the lowest (row,   */
/*             column) on a tie (pivoting on fixed columns would fail on a   */
/*             forward motion).  Null vector u, u < 4, is 1 at the u-th free */
/*             column, minus the reduced system's entries of that column at  */
/*             the pivot columns, 0 elsewhere; X, Y, Z, W are the rows of    */
/*             [1 -2 -3 -4; 2 1 -4 3; 3 4 1 -2; 4 -3 2 1] times the four,    */
/*             each scaled to unit length, and E = x X + y Y + z Z + W.      */
/*             det E = 0 and the nine entries of 2 E E' E - tr(E E') E = 0   */
/*             are the rows of a 10x20 matrix over the monomials x3 y3 x2y   */
/*             xy2 x2z x2 y2z y2 xyz xy xz2 xz x yz2 yz y z3 z2 z 1,         */
/*             eliminated on its first 10 columns with partial pivoting (the */
/*             largest |entry| of the column at or below the diagonal, the   */
/*             lowest row on a tie).  Rows 4..9 give three equations [3] x + */
/*             [3] y + [4] = 0 in polynomials of z; their determinant is the */
/*             degree-10 polynomial.  Its real roots: the Sturm sequence,    */
/*             counted at 256 equidistant points of [-B, B], B = min(1 + max */
/*             |a_i / a_n|, 1e12) (Cauchy); a cell with several roots is     */
/*             halved by Sturm counts (at most 64 times) until each root has */
/*             a cell with a change of sign, then bisection on the sign,     */
/*             ended when the midpoint is no longer inside or after 200      */
/*             steps.  (x, y, 1) is the cross product of the two equations   */
/*             with the largest third component; E is scaled to Frobenius    */
/*             norm sqrt(2).  Only + - * / and sqrt; every loop is bounded.  */
/*             0 models for a degenerate sample: a pivot not above 1e-12     */
/*             (5x9; a repeated correspondence) or 1e-13 (10x20), or a       */
/*             polynomial without a degree.  Models in ascending order of z. */
/*   error     of a correspondence under E: with u^ the camera model's       */
/*             pixel of a bearing with the distortion coefficients taken as  */
/*             zero, and F the matrix with u^_J' F u^_I proportional to      */
/*             b_J' E b_I: the squared distance in px of u^_J from the line  */
/*             F u^_I; +inf when it is not finite.                           */
/*   AC-RANSAC OpenMVG's ACRANSAC as sfm_fmatrix_ac restates it: the         */
/*             mt19937(default_seed) stream from position 0 per problem, the */
/*             same uniform_int restatement, two sampling modes, 10 %        */
/*             iteration reserve, focused resampling and tie rules.  A model */
/*             counts as found with more than 2.5 * 5 errors under the       */
/*             bound.  NFA(k) = loge0 + logalpha (k-5) + logcombi(k, n) +    */
/*             logcombi(5, k), k = 6 .. m, over the m errors under the bound */
/*             in ascending (error, index) order, logalpha = logalpha0 +     */
/*             0.5 log10(e_k + FLT_EPSILON), logalpha0 = log10(2 diag_J /    */
/*             area_J) of image J's size, loge0 = log10(10 (n - 5)); the two */
/*             logcombi tables are rounded to float, as OpenMVG's.  The      */
/*             bound is precision^2; precision <= 0 or +inf: none (every     */
/*             finite error).  Kept iff min_nfa < 0 and n_inliers > 12.      */
/*   motion    of a kept E, in closed form without an SVD (Horn 1990):       */
/*             t t' = tr(E E')/2 I - E E', t the row of its largest diagonal */
/*             entry (the first on a tie) over the root of that entry; with  */
/*             C the matrix of cofactors of E (rows e1 x e2, e2 x e0, e0 x   */
/*             e1 of E's rows), Ra = (C - [t]x E) / (t.t) and its twisted    */
/*             partner Rb = (C + [t]x E) / (t.t).  The four motions, in      */
/*             order: (Ra, t), (Ra, -t), (Rb, t), (Rb, -t).  For each, the   */
/*             inliers whose two-view triangulation (sfm_triangulate's       */
/*             linear solve of the two bearings under [I | 0] and [R | t])   */
/*             lies in front of both cameras are counted; in front is        */
/*             sfm_resect's: P2 > 0 (P2 < 0 for SNAVELY).  The motion with   */
/*             the largest count (the lowest index on a tie) wins iff the    */
/*             largest of the other three counts over it is below            */
/*             front_ratio; n_front is its count.  angle_median: the front   */
/*             inliers of the winner in ascending (|b_I - R' b_J|^2, index)  */
/*             order, the angle between b_I and R' b_J of the one at index   */
/*             n_front / 2, in degrees.  There is no refit: the two-view     */
/*             bundle adjustment is sfm_ba_solve's.                          */
/* status: SFM_RELPOSE_FEW (n <= 5, or fewer than 6 pairs of finite          */
/* bearings: everything 0), SFM_RELPOSE_NO_MODEL (not kept: everything 0 but */
/* iterations and min_nfa, the best seen, +inf when none),                   */
/* SFM_RELPOSE_AMBIGUOUS (E, error_max, min_nfa, n_inliers and the inliers   */
/* kept; the vote did not single out a motion: pose, n_front and             */
/* angle_median 0), SFM_RELPOSE_OK.  E = +-[t]x R up to rounding.            */
/* Two device runs give the same bits.  Host and device run the same         */
/* statements on every number of the search; they differ in the last bits of */
/* angle_median (atan2) only.                                                */
/* ------------------------------------------------------------------------ */
#define SFM_RELPOSE_OK        0
#define SFM_RELPOSE_FEW       1
#define SFM_RELPOSE_NO_MODEL  2
#define SFM_RELPOSE_AMBIGUOUS 3
typedef struct sfm_relpose_opts {
    double  precision;        /* px, upper bound of the a-contrario threshold; <= 0 or +inf: none */
    int32_t max_iterations;   /* 4096 (>= 1)                                                       */
    int32_t reserved;
    double  front_ratio;      /* 0.7: second-best / best cheirality count has to be below it       */
} sfm_relpose_opts;
typedef struct sfm_relpose_result {
    double  E[9];           /* row-major, on bearings: b_J' E b_I = 0, Frobenius norm sqrt(2) */
    double  pose[6];        /* angle-axis, then t, |t| = 1: P_J = R P_I + t                    */
    double  error_max;      /* px: square root of the a-contrario threshold                    */
    double  min_nfa;        /* log10 NFA of the best model                                     */
    double  angle_median;   /* degrees                                                         */
    int32_t n_inliers;
    int32_t n_front;
    int32_t iterations;     /* RANSAC iterations run                                           */
    int32_t status;         /* SFM_RELPOSE_*                                                   */
} sfm_relpose_result;
/* [cpu] {4.0, 4096, 0, 0.7}; NULL opts below select them. */
void sfm_relpose_default_options(sfm_relpose_opts* opts);
/* inliers[off[q] + t], t < results[q].n_inliers: the inliers (indices into
 * the problem's list) in ascending (error, index) order under E; the rest of
 * inliers[] is left alone.  Every argument check runs on the host before any
 * device call: a null pointer, negative counts, off[0] != 0 or off not
 * monotone, an unknown camera_model, pair_intr outside [0, n_intr), a
 * non-positive image size, max_iterations < 1 or a NaN precision or
 * front_ratio: SFM_ERR_INVALID_ARG; n_pairs or off[n_pairs] >= 2^31, or a
 * problem drawing more than 2^18 random numbers: SFM_ERR_UNSUPPORTED.
 * Problems of any size (the sort moves from LDS to global memory above 8192
 * correspondences).  It does not shard.  A context created with
 * SFM_CTX_TIME_KERNELS reports the kernel's device time through
 * sfm_ctx_last_kernel_ms. */
int sfm_relpose(sfm_ctx* ctx, int32_t camera_model, int64_t n_pairs, const int64_t* off /* [n_pairs+1] */,
                const double* xy /* [4*n] */, const int32_t* pair_intr /* [2*n_pairs] */,
                const double* intr /* [iw*n_intr] */, int32_t n_intr, const int32_t* wh /* [4*n_pairs] */,
                const sfm_relpose_opts* opts, sfm_relpose_result* results /* [n_pairs] */, int32_t* inliers /* [n] */);
/* [cpu] The same on the host, a serial loop over the same statements. */
int sfm_relpose_host(int32_t camera_model, int64_t n_pairs, const int64_t* off, const double* xy,
                     const int32_t* pair_intr, const double* intr, int32_t n_intr, const int32_t* wh,
                     const sfm_relpose_opts* opts, sfm_relpose_result* results, int32_t* inliers);
/* [cpu] The minimal solver alone: unit bearings bI[3i..], bJ[3i..], i < 5;
 * *n models, model m = E[m][0..8] row-major. */
int sfm_relpose_5pt(const double bI[15], const double bJ[15], double E[10][9], int32_t* n);

/* ------------------------------------------------------------------------ */
/* SIFT extraction: detect, orient and describe               */
/*                                                                           */
/* The first stage of the sparse pipeline: sparseBuilder::detectFeature()'s  */
/* SIFT_Image_describer over VLFeat's sift, on a batch of 8-bit gray images  */
/* of one size.  Image decoding stays outside: the input is gray bytes.      */
/*   scale space  first octave at the image's size (first_octave 0), then    */
/*             halved n_octaves - 1 times (every other pixel of level S);    */
/*             octaves run while both sides are at least 3.  Levels s = -1   */
/*             .. S+1 per octave, sigma0 = 1.6 * 2^(1/S), input blur 0.5;    */
/*             each level is the one below smoothed by a separable Gaussian  */
/*             of sqrt(sigma_s^2 - sigma_{s-1}^2), half-width ceil(4 sigma), */
/*             the border continued, columns first, float, taps added in     */
/*             order.  The taps are computed once on the host.               */
/*   detection    strict 3x3x3 extrema of the DoG at or beyond 0.8 peak,     */
/*             peak = 255 * peak_threshold / S; up to five steps of the 3-D  */
/*             quadratic fit (the cell moves when an offset passes 0.6);     */
/*             kept with |value| > peak, edge score below (e+1)^2 / e, every */
/*             offset below 1.5 and the point inside the octave.             */
/*   orientation  36 bins over a Gaussian window of 1.5 sigma, linear in the */
/*             angle, six 3-box passes, peaks at or above 0.8 of the largest */
/*             refined by a parabola, at most four, in bin order.            */
/*             orientation = 0: one upright feature (angle 0) per keypoint.  */
/*   descriptor   4x4x8 bins, magnification 3, window 2, trilinear; unit     */
/*             length, clamp at 0.2, unit length; then root_sift:            */
/*             (uint8)(512 sqrt(d / sum d)), else (uint8)(512 d).  A feature */
/*             whose centre rounds onto the last row of its octave gets a    */
/*             zero descriptor (the reference leaves its buffer as it was).  */
/*   arithmetic   gradient magnitude and angle and the two Gaussian windows  */
/*             use VLFeat's table / bit-trick replacements of sqrt, atan2    */
/*             and exp, restated as plain arithmetic (csrc/sift_point.h), so */
/*             host and device agree bit for bit; 2^x, sin and cos are short */
/*             Taylor sums.                                                  */
/* Features come in the reference's order: octave, then level, then row,     */
/* then column of the extremum cell, then orientations in bin order.  A      */
/* feature is (x, y, sigma, angle) in full-resolution pixels, float.         */
/* Limits: first_octave != 0 (the ULTRA preset's upsampling) and masks are   */
/* SFM_ERR_UNSUPPORTED / absent; n_scales <= 8; a Gaussian half-width above  */
/* 32 is SFM_ERR_UNSUPPORTED.                                                */
/* ------------------------------------------------------------------------ */
typedef struct sfm_sift_options {
    int32_t n_octaves;       /* 6                                             */
    int32_t n_scales;        /* 3 (S)                                         */
    int32_t first_octave;    /* 0; anything else: SFM_ERR_UNSUPPORTED         */
    float   edge_threshold;  /* 10                                            */
    float   peak_threshold;  /* 0.04 (NORMAL preset); HIGH: 0.01              */
    int32_t root_sift;       /* 1                                             */
    int32_t orientation;     /* 1                                             */
    int32_t reserved;
} sfm_sift_options;
typedef struct sfm_sift_summary {
    int64_t n_images;
    int64_t n_keypoints;     /* refined keypoints, before orientations        */
    int64_t n_features;      /* sum of n_feat                                 */
    int64_t n_written;       /* rows written: sum of min(n_feat, cap_per_img) */
    int64_t n_overflow;      /* images with n_feat > cap_per_img              */
    double  kernel_ms;       /* device time of the kernels; -1 without        */
                             /* SFM_CTX_TIME_KERNELS and on the host          */
} sfm_sift_summary;
/* [cpu] {6, 3, 0, 10, 0.04, 1, 1, 0}; NULL opts below select them. */
void sfm_sift_options_default(sfm_sift_options* opts);
/* gray: n_img images of w x h bytes, row-major, back to back.  Image i's
 * features go to xyso[i][0 .. ][4] and desc[i][0 .. ][128] in canonical order,
 * at most cap_per_img rows of them; n_feat[i] is always the true count, so
 * n_feat[i] > cap_per_img says that image i was cut short.  That is not an
 * error: the call returns SFM_OK and summary->n_overflow counts such images
 * (cap_per_img 0 with null xyso / desc is the size query).  Rows past the
 * count are left alone.  Every argument check runs on the host before any
 * device call: a null pointer, a negative count, a non-positive image size,
 * n_octaves < 0, n_scales < 1, edge_threshold <= 0 or peak_threshold < 0:
 * SFM_ERR_INVALID_ARG; the limits above, more than 2^28 pixels per image or
 * 65535 images: SFM_ERR_UNSUPPORTED.  n_img 0 and images smaller than 3 x 3
 * give no features.  Two device runs, and device and host, give the same bits.
 * It does not shard.  summary may be NULL.  A context created with
 * SFM_CTX_TIME_KERNELS also reports the kernels' device time through
 * sfm_ctx_last_kernel_ms. */
int sfm_sift(sfm_ctx* ctx, const uint8_t* gray, int32_t n_img, int32_t w, int32_t h, const sfm_sift_options* opts,
             int64_t cap_per_img, float* xyso /* [n_img][cap][4] */, uint8_t* desc /* [n_img][cap][128] */,
             int64_t* n_feat /* [n_img] */, sfm_sift_summary* summary);
/* [cpu] The same on the host, a serial loop over the same statements. */
int sfm_sift_host(const uint8_t* gray, int32_t n_img, int32_t w, int32_t h, const sfm_sift_options* opts,
                  int64_t cap_per_img, float* xyso, uint8_t* desc, int64_t* n_feat, sfm_sift_summary* summary);

/* ------------------------------------------------------------------------ */
/* Incremental reconstruction                                 */
/* OpenMVG's SequentialSfMReconstructionEngine::Process() as reconstruction() */
/* runs it (sparseBuilder.cpp:1283-1599: engine INCREMENTAL,                 */
/* PINHOLE_CAMERA_RADIAL3, ADJUST_ALL), over the batch stages above.         */
/* Restated from its published code, parity unpinned.         */
/*                                                                          */
/* Round queries.  The tracks do not change between rounds: a                */
/* sfm_recon_tracks handle holds a sfm_ba_problem's structure (pt_offsets,   */
/* obs_img, obs_uv) on the device (or, for the host twin, on the host) and   */
/* answers three questions about the per-round state registered[n_img],      */
/* pt_ok[n_pt] (uint8, != 0 is set) and X[3*n_pt].  An observation is alive  */
/* until sfm_recon_tracks_drop_obs names it.  Every output is integral or a  */
/* gather: a device handle and a host handle give the same bytes.            */
/*   visibility  count[i] = the points p with pt_ok[p] that have at least    */
/*               one alive observation in image i (two observations of one   */
/*               point in one image count once), for every image.            */
/*   gather      sfm_resect_gather over alive observations: for the images   */
/*               listed, off[n_images+1] and X3 / uv, image by image, each   */
/*               image's correspondences in the problem's observation order. */
/*   select      the sub-problem of the alive observations whose image is    */
/*               registered, over the points that qualify: SFM_RECON_NEW     */
/*               pt_ok[p] == 0 and two such observations in different        */
/*               images; SFM_RECON_SOLVED pt_ok[p] != 0 and at least         */
/*               min_track_len (>= 1) such observations.  Points keep their  */
/*               order and each point's observations theirs; pt_map[k] /     */
/*               obs_map[k] = the old index of new point / observation k.    */
/*                                                                          */
/* The driver.  sfm_reconstruct(tracks, intr, wh, pairs):                    */
/*   pair      every candidate pair (I, J) of pairs[]: its correspondences   */
/*             are the tracks holding both images, in track order (an        */
/*             image's first observation in the track); one sfm_relpose call */
/*             over all pairs; the pair is the one the engine's rule picks   */
/*             (status OK, n_front > pair_min_inliers, angle_median >        */
/*             pair_min_angle_deg, the largest angle_median, the first on a  */
/*             tie).  initial_pair[0] >= 0 names the pair instead: it only   */
/*             has to come out SFM_RELPOSE_OK.  No pair: SFM_OK with         */
/*             stats->status = SFM_RECON_NO_INITIAL_PAIR, nothing            */
/*             registered.  Image I gets the identity, image J the result;   */
/*             then `points` below.  No bundle adjustment runs on the pair   */
/*             alone (OpenMVG adjusts it with the intrinsics held fixed;     */
/*             this library has no fixed-intrinsics solve and two views with */
/*             free intrinsics are ill-posed).                               */
/*   round     visibility; best = the largest count over the images neither  */
/*             registered nor tried; 0 ends the loop.  Candidates: those     */
/*             images with count >= group_ratio * best, ascending; gather,   */
/*             one sfm_resect call; every candidate is tried for good; those */
/*             that come out SFM_RESECT_OK are registered at the refined     */
/*             pose, and their correspondences outside the resection's       */
/*             inliers are dropped for good (the engine adds the inliers to  */
/*             its landmarks, nothing else).  Then `points`, then `adjust`.  */
/*   points    select(NEW) -> sfm_triangulate(tri).  An OK point sets pt_ok  */
/*             and X; its observations the triangulation did not keep are    */
/*             dropped for good.                                             */
/*   adjust    (adjust != 0) select(SOLVED, min_track_len) -> sfm_ba_solve   */
/*             (const_img = image I of the pair, the tracks' huber_a) ->     */
/*             sfm_ba_wash(wash).  A removed point gets pt_ok = 0, X = NaN   */
/*             and may be triangulated again; a rejected observation of a    */
/*             surviving point is dropped for good.  Repeats while the wash  */
/*             took more than wash_repeat_above observations out of the      */
/*             sub-problem, at most max_adjust_repeats times.  A solve that  */
/*             is not usable leaves everything as it was and ends the step.  */
/*             An observation whose image is registered after its point was  */
/*             solved enters the next select(SOLVED); the wash judges it.    */
/*   end       (adjust != 0) one more `adjust` with wash_repeat_above = 0.   */
/* Round 0 of the log is the pair (two candidates: the images, count = the   */
/* common tracks, status / n_inliers the relative pose's).  rounds[] and     */
/* cands[] take what fits; stats->n_rounds / n_cands are the true counts.    */
/* sfm_reconstruct_host runs the same driver over the host twins; the        */
/* library has no host bundle adjustment, so adjust != 0 there is            */
/* SFM_ERR_UNSUPPORTED.  With adjust == 0 both take the same decisions.      */
/* ------------------------------------------------------------------------ */
typedef struct sfm_recon_tracks sfm_recon_tracks;
#define SFM_RECON_NEW    0
#define SFM_RECON_SOLVED 1
/* Argument checks (host, before any device call): a null pointer, negative
 * counts, pt_offsets not running monotonically from 0 to n_obs, an image
 * outside [0, n_img): SFM_ERR_INVALID_ARG; n_pt or n_obs >= 2^31 - 1:
 * SFM_ERR_UNSUPPORTED.  img_intr, const_img, camera_model are not read. */
int sfm_recon_tracks_create(sfm_ctx* ctx, const sfm_ba_problem* prob, sfm_recon_tracks** out);
/* [cpu] the host twin of the handle */
int sfm_recon_tracks_create_host(const sfm_ba_problem* prob, sfm_recon_tracks** out);
int sfm_recon_tracks_destroy(sfm_recon_tracks* t);
/* obs[n]: observations (old indices) that are no longer alive. */
int sfm_recon_tracks_drop_obs(sfm_recon_tracks* t, const int64_t* obs, int64_t n);
int sfm_recon_visibility(sfm_recon_tracks* t, const uint8_t* pt_ok, int32_t* count /* [n_img] */);
/* off[n_images+1] is always the true layout; X3[3*cap] / uv[2*cap] are
 * written only when off[n_images] <= cap (cap 0 with NULL arrays: the size
 * query); obs[cap] (optional, with them): each row's old observation index.  An image out of range or listed twice: SFM_ERR_INVALID_ARG. */
int sfm_recon_gather(sfm_recon_tracks* t, const double* X, const uint8_t* pt_ok, const int32_t* images,
                     int32_t n_images, int64_t* off, double* X3, double* uv, int64_t* obs, int64_t cap);
/* *n_pt_out / *n_obs_out are always the true sizes; pt_offsets[cap_pt+1],
 * pt_map[cap_pt], obs_img / obs_map[cap_obs], obs_uv[2*cap_obs] are written
 * only when both fit (caps 0 with NULL arrays: the size query). */
int sfm_recon_select(sfm_recon_tracks* t, const uint8_t* registered, const uint8_t* pt_ok, int32_t mode,
                     int32_t min_track_len, int64_t* n_pt_out, int64_t* n_obs_out, int64_t* pt_offsets,
                     int32_t* obs_img, double* obs_uv, int64_t* pt_map, int64_t* obs_map, int64_t cap_pt,
                     int64_t cap_obs);

#define SFM_RECON_OK              0
#define SFM_RECON_NO_INITIAL_PAIR 1
typedef struct sfm_recon_opts {
    sfm_relpose_opts relpose;     /* sfm_relpose_default_options                  */
    sfm_resect_opts  resect;      /* sfm_resect_default_options                   */
    sfm_tri_opts     tri;         /* sfm_tri_default_options                      */
    sfm_ba_options   ba;          /* sfm_ba_default_options                       */
    sfm_ba_wash_opts wash;        /* sfm_ba_wash_default_options                  */
    int32_t initial_pair[2];      /* {-1, -1}: automatic                          */
    int32_t pair_min_inliers;     /* 100                                          */
    int32_t adjust;               /* 1                                            */
    double  pair_min_angle_deg;   /* 3.0                                          */
    double  group_ratio;          /* 0.75 (dThresholdGroup)                       */
    int32_t wash_repeat_above;    /* 50                                           */
    int32_t max_adjust_repeats;   /* 8 (>= 1)                                     */
    int32_t min_track_len;        /* 2 (>= 1): select(SOLVED)                     */
    int32_t reserved;
} sfm_recon_opts;
typedef struct sfm_recon_cand {
    int32_t round, image;
    int32_t count;                /* visibility count (round 0: common tracks)    */
    int32_t status;               /* SFM_RESECT_* (round 0: SFM_RELPOSE_*)        */
    int32_t n_inliers, reserved;
} sfm_recon_cand;
typedef struct sfm_recon_round {
    int32_t first_cand, n_cand;   /* cands[first_cand .. first_cand + n_cand)     */
    int32_t n_registered;         /* candidates registered in this round          */
    int32_t adjust_repeats;       /* solves run (0: none)                          */
    int64_t points_added;         /* triangulated OK                              */
    int64_t obs_dropped;          /* by the triangulation and the washes          */
    int64_t points_removed;       /* by the washes                                */
    int32_t ba_rc, reserved;      /* the last solve's return code                 */
    sfm_ba_summary ba;            /* the last solve                               */
    sfm_ba_wash_stats wash;       /* the last wash                                */
} sfm_recon_round;
typedef struct sfm_recon_stats {
    int32_t status;               /* SFM_RECON_*                                  */
    int32_t initial_pair[2];      /* (I, J); -1 without                           */
    int32_t n_rounds, n_cands;    /* true counts (the log may hold fewer)         */
    int32_t n_registered;
    int64_t n_points, n_obs_kept;
    int64_t final_removed;        /* observations the last wash took out          */
    sfm_recon_round final_adjust; /* the closing adjustment (adjust != 0)         */
    double seconds[8];            /* wall: pair search, visibility, gather,
                                     select, resect, triangulate, solve, wash    */
} sfm_recon_stats;
/* [cpu] the defaults above; NULL opts below select them. */
void sfm_recon_default_options(sfm_recon_opts* opts);
/* tracks: n_img, n_intr, n_pt, n_obs, pt_offsets, obs_img, obs_uv, img_intr,
 * camera_model, huber_a (const_img is ignored).  intr[iw*n_intr] in / out
 * (refined when adjust != 0), wh[2*n_img], pairs[2*n_pairs].  Outputs:
 * extr[6*n_img] (0 for an unregistered image), X[3*n_pt] (NaN where the point
 * is not reconstructed), registered[n_img], pt_ok[n_pt], keep_obs[n_obs] (the
 * alive observations of reconstructed points in registered images); rounds /
 * cands may be NULL with cap 0, stats may be NULL.  Every argument check runs
 * on the host before any device call: the checks of sfm_recon_tracks_create,
 * img_intr outside [0, n_intr), an unknown camera_model, a non-positive image
 * size, a pair naming an image out of range or twice, negative capacities,
 * group_ratio outside (0, 1], max_adjust_repeats or min_track_len < 1, and
 * the stages' option checks: SFM_ERR_INVALID_ARG.  It does not shard. */
int sfm_reconstruct(sfm_ctx* ctx, const sfm_ba_problem* tracks, double* intr, const int32_t* wh,
                    const int32_t* pairs, int64_t n_pairs, const sfm_recon_opts* opts, double* extr, double* X,
                    uint8_t* registered, uint8_t* pt_ok, uint8_t* keep_obs, sfm_recon_round* rounds,
                    int32_t cap_rounds, sfm_recon_cand* cands, int32_t cap_cands, sfm_recon_stats* stats);
/* [cpu] */
int sfm_reconstruct_host(const sfm_ba_problem* tracks, double* intr, const int32_t* wh, const int32_t* pairs,
                         int64_t n_pairs, const sfm_recon_opts* opts, double* extr, double* X,
                         uint8_t* registered, uint8_t* pt_ok, uint8_t* keep_obs, sfm_recon_round* rounds,
                         int32_t cap_rounds, sfm_recon_cand* cands, int32_t cap_cands, sfm_recon_stats* stats);

/* sparseBuilder::reconstruction(), file-staged: sfm_data.json (views, sizes)
 * + <stem>.feat + matches.f.bin -> sfm_sparse_tracks -> sfm_reconstruct with
 * SFM_CAM_RADIAL3, one intrinsics block per view {focal, w/2, h/2, 0, 0, 0}
 * (focal <= 0: 1.2 * max(w, h), OpenMVG's guess without EXIF), the candidate
 * pairs those of the matches file -> <out_dir>/cloud_and_poses.ply in the
 * layout of OpenMVG's plyHelper::exportToPly: ASCII, double x y z + uchar
 * red green blue, the points in white, then the camera centres in green.
 * sfm_data.bin (cereal binary) is not written.  opts NULL = the defaults. */
int sfm_sparse_reconstruct(sfm_ctx* ctx, const char* matches_dir, const char* out_dir, double focal,
                           const sfm_recon_opts* opts, sfm_recon_stats* stats);

/* ------------------------------------------------------------------------ */
/* Track colouring                                           */
/* sparseBuilder::colorize() (sparseBuilder.cpp:1601-1630): OpenMVG's        */
/* ColorizeTracks, a greedy cover.  While uncoloured points remain: count    */
/* for every view how many of them it sees, take the view that sees the      */
/* most, give each of those points the pixel under its observation in that   */
/* view.  Restated from its published description.                           */
/*                                                                          */
/* Inputs: the tracks as in sfm_ba_problem (n_img, n_pt, n_obs, pt_offsets,  */
/* obs_img, obs_uv; nothing else is read), wh[2*n_img], pt_ok[n_pt] (the     */
/* points to colour; NULL: all), keep_obs[n_obs] (the live observations;     */
/* NULL: all): what sfm_reconstruct returns.  A point is to colour when      */
/* pt_ok says so and it has a live observation.  A point counts once per     */
/* image (OpenMVG's Observations is a map keyed by view): of several live    */
/* observations of a track in one image the first in track order is used.    */
/*   count[v]  the still uncoloured points to colour with a live             */
/*             observation in v.                                             */
/*   round     v = the view with the largest count; a tie goes to the lowest */
/*             image index (OpenMVG sorts with std::sort, which leaves ties  */
/*             unspecified; this library fixes them).  Every uncoloured      */
/*             point seen in v gets view[p] = v, obs[p] = the observation    */
/*             used, px[2p..] = ((int)clamp(u, 0, w-1), (int)clamp(v, 0,     */
/*             h-1)), the clamp in double, then truncation, and leaves the   */
/*             set.  The rounds stop when no count is positive.              */
/* Outputs: view[n_pt] (-1 where the point is not coloured), obs[n_pt] (-1   */
/* likewise), px[2*n_pt] (0 0 likewise), order[n_img] (the chosen views in   */
/* order, -1 from n_rounds on), *n_rounds.  All integers: the device and the */
/* host twin give the same bytes.                                            */
/* The device chooses, the host samples: choosing is the whole cost (integer */
/* work over the tracks), sampling is one pixel per point from images that   */
/* are far too large to upload for that; and an image is needed only once a  */
/* round has chosen it.  The device keeps count[] incrementally (a coloured  */
/* point takes 1 off every image it is seen in) instead of recounting every  */
/* round: O(n_obs + rounds * n_img) work.                                    */
/* ------------------------------------------------------------------------ */
typedef struct sfm_colorize_stats {
    int64_t n_to_colour;          /* points with pt_ok and a live observation     */
    int64_t n_coloured;           /* points with view >= 0                        */
    int32_t n_rounds, reserved;
    double seconds[3];            /* wall: index build (and upload), rounds,
                                     download                                     */
} sfm_colorize_stats;
/* Every argument check runs on the host before any device call, and every
 * violation is SFM_ERR_INVALID_ARG with a message: the checks of
 * sfm_recon_tracks_create; n_pt or n_obs >= 2^31 - 1; a non-positive image
 * size; a non-finite uv on a live observation of a point to colour.  stats may
 * be NULL. */
int sfm_colorize_assign(sfm_ctx* ctx, const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                        const uint8_t* keep_obs, int32_t* view, int64_t* obs, int32_t* px, int32_t* order,
                        int32_t* n_rounds, sfm_colorize_stats* stats);
/* [cpu] the serial twin */
int sfm_colorize_assign_host(const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                             const uint8_t* keep_obs, int32_t* view, int64_t* obs, int32_t* px, int32_t* order,
                             int32_t* n_rounds, sfm_colorize_stats* stats);
/* [cpu] rgb[3p..] = the pixel of image view[p] at px[2p..]; 0 0 0 where
 * view[p] < 0.  pixels is one byte pool: image i starts at byte img_off[i]
 * (< 0: the caller did not load it), row-major, interleaved, row stride
 * w * channels[i], channels[i] 1 (gives g g g) or 3 (read for loaded images
 * only).  SFM_ERR_INVALID_ARG: a view outside [-1, n_img), a px outside its
 * image, channels not 1 or 3, an unloaded image that some view[p] names. */
int sfm_colorize_sample(int64_t n_pt, const int32_t* view, const int32_t* px, int32_t n_img, const int32_t* wh,
                        const int32_t* channels, const int64_t* img_off, const uint8_t* pixels, uint8_t* rgb);
/* Assign and sample in one call: rgb[3*n_pt]; view[n_pt] is optional (NULL).
 * Beyond the checks above, before any device call: channels of a loaded image
 * not 1 or 3, an unloaded image that has a live observation of a point to
 * colour: SFM_ERR_INVALID_ARG. */
int sfm_colorize(sfm_ctx* ctx, const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                 const uint8_t* keep_obs, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                 uint8_t* rgb, int32_t* view, sfm_colorize_stats* stats);
/* [cpu] */
int sfm_colorize_host(const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                      const uint8_t* keep_obs, const int32_t* channels, const int64_t* img_off,
                      const uint8_t* pixels, uint8_t* rgb, int32_t* view, sfm_colorize_stats* stats);
/* [cpu] colorized.ply, in the layout sfm_sparse_reconstruct writes: ASCII,
 * double x y z ("%.16f") + uchar red green blue, the points with pt_ok (NULL:
 * all) ascending, each in its colour rgb[3p..] (rgb NULL: white), then the
 * centres C = -R' t of the registered (NULL: all) cameras in green. */
int sfm_colorize_write_ply(const char* path, int64_t n_pt, const double* X, const uint8_t* pt_ok,
                           const uint8_t* rgb, int32_t n_img, const double* extr, const uint8_t* registered);
/* sparseBuilder::reconstruction() + colorize(), file-staged:
 * sfm_sparse_reconstruct, then sfm_colorize over the pt_ok / keep_obs it
 * returned, with the views of sfm_data.json as the images (channels, img_off,
 * pixels as above, in the file's view order).  Writes
 * <out_dir>/cloud_and_poses.ply (the same bytes as sfm_sparse_reconstruct) and
 * <out_dir>/colorized.ply.  One call, because sfm_data.bin is not written: no
 * file carries the scene from one stage to the next.  Either stats may be
 * NULL. */
int sfm_sparse_reconstruct_colorize(sfm_ctx* ctx, const char* matches_dir, const char* out_dir, double focal,
                                    const sfm_recon_opts* opts, const int32_t* channels, const int64_t* img_off,
                                    const uint8_t* pixels, sfm_recon_stats* recon_stats,
                                    sfm_colorize_stats* color_stats);

/* ------------------------------------------------------------------------ */
/* Dense hand-off                                            */
/* What denseWork() does before any MVS runs (OpenMVG's openMVG2openMVS      */
/* export; src/denseBuilder/DenseBuilder.h:54-146 collects the same scene):  */
/* every image is undistorted, and the scene (platforms with a               */
/* distortion-free K, one image and pose per registered view, one vertex per */
/* point seen in two or more of them) is collected.  The undistortion is     */
/* per-pixel resampling of every image and runs on the device; the scene is  */
/* integer work over the tracks and stays on the host.                       */
/*                                                                          */
/* Images: as sfm_colorize_sample reads them.  One byte pool `pixels`, image */
/* i of wh[2i..] = (w, h) and channels[i] (1 or 3) starts at byte img_off[i] */
/* (< 0: not loaded, skipped), row-major, interleaved, no row padding; the   */
/* offsets need no alignment.  `out` has the same layout and offsets; bytes  */
/* outside the loaded images are not touched.  Cameras: camera_model,        */
/* img_intr[n_img], intr[iw*n_intr].                                         */
/*   SFM_CAM_PINHOLE  no distortion: the image is a byte copy (OpenMVG       */
/*                    copies the file).                                      */
/*   SFM_CAM_RADIAL3  resampled whatever k1..k3 are (OpenMVG's have_disto()  */
/*                    is a property of the class).                           */
/*   SFM_CAM_SNAVELY  SFM_ERR_UNSUPPORTED: the BAL model has no principal    */
/*                    point and so no raster origin.                         */
/* Per pixel (OpenMVG's UndistortImage with Sampler2d<SamplerLinear>,        */
/* restated from the published source).  For the output pixel (i, j) and     */
/* {f, ppx, ppy, k1, k2, k3}, in double and in this order:                   */
/*   px = (i - ppx) / f, py = (j - ppy) / f, r2 = px*px + py*py,             */
/*   r4 = r2*r2, r6 = r4*r2, c = 1.0 + k1*r2 + k2*r4 + k3*r6,                */
/*   x = f*(px*c) + ppx, y = f*(py*c) + ppy.                                 */
/* The source is inside when x > -1.0 && x < w && y > -1.0 && y < h (NaN     */
/* fails); otherwise the pixel is `fill`.  Inside: xf = (float)x,            */
/* gx = floorf(xf), dx = (double)xf - (double)gx, likewise yf, gy, dy; the   */
/* weights are {1 - dx, dx} and {1 - dy, dy}.  Over the rows gy, gy + 1      */
/* (outer) and the columns gx, gx + 1 (inner), neighbours outside the image  */
/* skipped: res += (double)pix * (wx*wy) per channel, total += wx*wy.        */
/* total <= 0.2: the pixel is 0 in every channel (not `fill`).  Otherwise    */
/* res /= total when total != 1.0, and the byte is (uint8_t)(res + 0.5).     */
/* No operation is fused (csrc/undistort_point.h, one definition for the     */
/* kernel and the host twin), so the device and the host twin give the same  */
/* bytes and the same counts.                                                */
/* ------------------------------------------------------------------------ */
typedef struct sfm_undistort_opts {
    int64_t chunk_bytes;     /* the device working set of one chunk (pitched
                                input and output rows), so that a collection
                                larger than device memory streams through;
                                0: the library's default, 128 MiB.  Two chunks
                                are resident at a time.  The result does not
                                depend on it.                                  */
    uint8_t fill[3];         /* the pixel whose source falls outside (0 0 0);
                                a 1-channel image takes fill[0]                */
    uint8_t reserved[5];
} sfm_undistort_opts;
/* [cpu] chunk_bytes 0, fill black */
void sfm_undistort_default_options(sfm_undistort_opts* opts);
typedef struct sfm_undistort_stats {
    int64_t n_images;        /* loaded images (resampled or copied)            */
    int64_t n_copied;        /* of those, byte copies (SFM_CAM_PINHOLE)        */
    int64_t n_pixels;        /* output pixels of the resampled images          */
    int64_t n_outside;       /* of those, the source fell outside: `fill`      */
    int64_t n_low_weight;    /* of those, inside with total <= 0.2: 0          */
    int32_t n_chunks;        /* chunks of the plan (the host twin reports the
                                plan the device would run)                    */
    int32_t reserved;
    double seconds[3];       /* upload, kernels, download.  Device: summed over
                                the chunks from stream events (chunks overlap,
                                so the sum may exceed the wall time).  Host
                                twin: 0, the resampling's wall time, 0.        */
} sfm_undistort_stats;
/* Every argument check runs on the host before any device call, and every
 * violation is SFM_ERR_INVALID_ARG with a message: a non-positive image size,
 * channels other than 1 or 3 on a loaded image, img_intr out of range, an
 * unknown model, non-finite intrinsics or f == 0 on a block that a loaded
 * image uses, a positive chunk_bytes too small for one output row of an image
 * and the source rows it samples.  An image of 2^31 or more pixels is
 * SFM_ERR_UNSUPPORTED.  Chunks split between images and, for an image larger
 * than the budget, between rows (the source rows each band samples are worked
 * out on the host with the same arithmetic).  n_img == 0, or nothing loaded,
 * succeeds and writes nothing.  opts NULL = the defaults; stats may be NULL. */
int sfm_undistort(sfm_ctx* ctx, int32_t camera_model, int32_t n_img, int32_t n_intr, const int32_t* img_intr,
                  const double* intr, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                  const uint8_t* pixels, const sfm_undistort_opts* opts, uint8_t* out, sfm_undistort_stats* stats);
/* [cpu] the host twin (threads over bands of rows): the same bytes and counts */
int sfm_undistort_host(int32_t camera_model, int32_t n_img, int32_t n_intr, const int32_t* img_intr,
                       const double* intr, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                       const uint8_t* pixels, const sfm_undistort_opts* opts, uint8_t* out,
                       sfm_undistort_stats* stats);
/* [cpu] one image as binary PNM: "P5" (channels 1) or "P6" (channels 3),
 * maxval 255.  Needs no codec; image encoding otherwise stays outside the
 * library. */
int sfm_undistort_write_pnm(const char* path, int32_t w, int32_t h, int32_t channels, const uint8_t* bytes);

/* The scene of openMVG2openMVS / DenseBuilder::save(), from what
 * sfm_reconstruct returns: tracks (n_img, n_intr, n_pt, n_obs, pt_offsets,
 * obs_img, img_intr, camera_model are read), intr[iw*n_intr], extr[6*n_img],
 * X[3*n_pt], wh[2*n_img]; registered[n_img], pt_ok[n_pt], keep_obs[n_obs] may
 * each be NULL: all.
 *   platforms  one per intrinsics block, in block order, used or not.  K is
 *              row-major: PINHOLE [fx 0 cx; 0 fy cy; 0 0 1], RADIAL3
 *              [f 0 ppx; 0 f ppy; 0 0 1] (no distortion: the images are
 *              undistorted), SNAVELY SFM_ERR_UNSUPPORTED.  platform_wh is the
 *              size of the lowest-indexed image of the block (0 0: none);
 *              images of one block with different sizes: SFM_ERR_INVALID_ARG.
 *   images     the registered images in ascending index order get the scene
 *              IDs 0, 1, ...: image_src (the index), image_platform,
 *              image_pose (the rank among the registered images of its
 *              platform), R = R(w) row-major, C = -R' t.
 *   vertices   for each point with pt_ok, in point order: the scene IDs of
 *              the registered images that hold a live observation of it, each
 *              once, ascending.  Fewer than two: dropped and counted in
 *              n_short.  vert_X is X as float, vert_pt the source point,
 *              vert_off[n_vertices + 1] / vert_view[n_views] the lists (CSR).
 * Non-finite X or extr on something kept, or non-finite intr:
 * SFM_ERR_INVALID_ARG.  The OpenMVS .mvs archive is not written (DESIGN.md
 * §10); these arrays are everything it holds for this step. */
typedef struct sfm_dense_scene sfm_dense_scene;
typedef struct sfm_dense_scene_info {
    int32_t n_platforms, n_images;
    int64_t n_vertices, n_views, n_short;
} sfm_dense_scene_info;
/* [cpu] */
int sfm_dense_scene_build(const sfm_ba_problem* tracks, const double* intr, const double* extr, const double* X,
                          const int32_t* wh, const uint8_t* registered, const uint8_t* pt_ok,
                          const uint8_t* keep_obs, sfm_dense_scene** scene);
/* [cpu] */
int sfm_dense_scene_get_info(const sfm_dense_scene* scene, sfm_dense_scene_info* info);
/* [cpu] fills each array that is non-NULL: K[9*n_platforms],
 * platform_wh[2*n_platforms], image_src / image_platform / image_pose
 * [n_images], R[9*n_images], C[3*n_images], vert_X[3*n_vertices],
 * vert_off[n_vertices + 1], vert_view[n_views], vert_pt[n_vertices]. */
int sfm_dense_scene_fetch(const sfm_dense_scene* scene, double* K, int32_t* platform_wh, int32_t* image_src,
                          int32_t* image_platform, int32_t* image_pose, double* R, double* C, float* vert_X,
                          int64_t* vert_off, uint32_t* vert_view, int64_t* vert_pt);
/* [cpu] */
int sfm_dense_scene_destroy(sfm_dense_scene* scene);

/* ------------------------------------------------------------------------ */
/* Dense depth maps                                          */
/* The first half of denseWork()'s second command, DensifyPointCloud: which  */
/* views each image is matched against, a depth and a normal per pixel by    */
/* PatchMatch stereo on the device, and the cross-view consistency filter.   */
/* OpenMVS is not available here, so nothing below is pinned to its numbers: */
/* this comment is the contract.  The scheme is the red/black checkerboard   */
/* PatchMatch of Gipuma / ACMH (the family OpenMVS's GPU path belongs to): a */
/* pass updates the pixels of one colour from planes of the other colour     */
/* only, so it has no races and no order, and the device, the host twin and  */
/* a restatement give the same bytes.  Fusion, .dmap / .mvs files and the    */
/* mesh stage are not built.                                                 */
/*                                                                          */
/* Images: n_img images laid out as sfm_undistort's `out` (wh, channels 1 or */
/* 3, img_off < 0: not loaded, one byte pool).  A 3-channel pixel becomes    */
/* gray by (77 r + 150 g + 29 b + 128) >> 8.  Cameras per image: K[9], R[9]  */
/* row-major, C[3]: x = K R (X - C).  Neighbours: CSR nb_off[n_img + 1],     */
/* nb_view (at most 8 per image); drange[2 i ..] = d_min, d_max (float).     */
/* Maps: image i's maps start at pixel map_off(i) = the sum of w * h of the  */
/* images before it, loaded or not: depth[n_map], normal[3 n_map],           */
/* cost[n_map].  An image gets maps when it is loaded and has neighbours     */
/* ("active"); every other image's maps are all zero.  In an active image    */
/* the pixels at least r = half_window from every edge are estimated; the    */
/* others are depth 0, normal 0 0 0, cost 2.                                 */
/*                                                                          */
/* All per-pixel arithmetic is float, every operation a single IEEE          */
/* operation in the order written; a (x) b (+) c stands for two operations.  */
/* dot(a, b) = (a0 b0 + a1 b1) + a2 b2.  M [x y 1] has the rows              */
/* (M0 x + M1 y) + M2.  The host works out in double and rounds once, per    */
/* image Ki = K^-1 and per (reference r, neighbour j)                        */
/*   A = K_j R_j R_r' K_r^-1,  b = K_j R_j (C_r - C_j).                      */
/* ray(q) = Ki [q 1].  imin = 1.0f / d_max, imax = 1.0f / d_min.             */
/* Plane (d, n) at pixel p: t = dot(n, d * ray(p)) (d times each component). */
/* For a patch pixel q: z = t / dot(n, ray(q)), a = A [q 1],                 */
/* h = z * a + b (per component), x = h0 / h2, y = h1 / h2.  The sample is   */
/* valid when z > 0, h2 > 0, 0 <= x <= w_j - 1, 0 <= y <= h_j - 1 (NaN       */
/* fails).  x0 = floorf(x), fx = x - x0, x1 = min(x0 + 1, w_j - 1), likewise */
/* y; top = g00 + fx * (g10 - g00), bot = g01 + fx * (g11 - g01),            */
/* sample = top + fy * (bot - top).                                          */
/* Cost against one neighbour: over the (2r+1)^2 = N patch, rows outer,      */
/* columns inner, a = the reference's gray at the integer pixel, b = the     */
/* sample: Sa += a, Sb += b, Saa += a a, Sbb += b b, Sab += a b.             */
/* va = Saa - (Sa Sa) / N, vb = Sbb - (Sb Sb) / N, cov = Sab - (Sa Sb) / N.  */
/* Any invalid sample, !(va >= N), !(vb >= N) or a neighbour that is not     */
/* loaded: cost 2.  Otherwise c = cov / sqrtf(va * vb) clamped to [-1, 1]    */
/* and cost = 1 - c.                                                         */
/* Cost of a plane: the neighbours' costs ascending, the first               */
/* m = min(n_best, n_nb) summed in that order, divided by (float)m.          */
/* Random numbers: draw k of pixel idx = y w + x of image i is               */
/*   u_k = (float)(mix64(entity_seed(seed, i, idx) + k * 0x9E3779B97F4A7C15) */
/*                 >> 40) * 2^-24   (csrc/synth_rng.h's mix64, entity_seed). */
/* Draws 0 1 2: the initial plane.  Iteration it (from 0) uses               */
/* 3 + 7 it + {0: depth, 1 2 3: normal} for the perturbed plane and          */
/* 3 + 7 it + {4 5 6} for the fresh random plane.                            */
/* Random plane from (u, u', u''): inv = imin + u * (imax - imin),           */
/* d = 1.0f / inv, n = (2 u' - 1, 2 u'' - 1, -1) divided by its length       */
/* sqrtf((n0 n0 + n1 n1) + n2 n2), negated when dot(n, ray(p)) > 0.          */
/* Init: the random plane, or the caller's (init_depth, init_normal, used    */
/* as they are: a plane that is no plane costs 2); its cost.                 */
/* Iteration it: the pixels with (x + y) & 1 == 0, then the others.  At an   */
/* active pixel p with plane (d, n) and cost c:                              */
/*   1. for the offsets (-1,0) (1,0) (0,-1) (0,1) (-5,0) (5,0) (0,-5) (0,5)  */
/*      in this order, where p + offset = s is an estimated pixel: with s's  */
/*      plane (d_s, n_s), d' = dot(n_s, d_s * ray(s)) / dot(n_s, ray(p));    */
/*      skipped unless d_min <= d' <= d_max (NaN fails); the plane (d', n_s) */
/*      replaces the current one when its cost is strictly lower.            */
/*   2. delta = 0.1f / 2^it; inv = 1.0f / d + (delta * (2 u - 1)) * (imax -  */
/*      imin) clamped to [imin, imax], d' = 1.0f / inv; n' = n + delta *     */
/*      (2 u_c - 1) per component, divided by its length, facing rule as     */
/*      above; taken when strictly lower.                                    */
/*   3. a fresh random plane; taken when strictly lower.                     */
/* No operation is fused (csrc/depthmap_point.h, one definition for the      */
/* kernels and the host twin).                                               */
/*                                                                          */
/* View selection (after OpenMVS's published SelectNeighborViews, restated   */
/* from memory: the weights and defaults are this library's design choices,  */
/* not its numbers).  For image i and every other image j, over the vertices */
/* seen in both, in double: theta = the angle at X between C_i - X and       */
/* C_j - X in degrees; w_angle = min(theta / opt_angle, 1)^1.5;              */
/* s = (f_i / z_i) / (f_j / z_j) with f = K[0] and z the depth of X in each  */
/* camera; w_scale = s^2 if s < 1, (max_scale / s)^2 if s > max_scale, else  */
/* 1; score(i, j) = the sum of w_angle * w_scale.  j is dropped when fewer   */
/* than min_shared vertices are shared or the mean theta is below min_angle; */
/* the rest sorted by score descending, ties to the lower index, at most     */
/* max_neighbors (<= 8) kept.  drange = z_min / (1 + m), z_max * (1 + m)     */
/* over the positive depths of the image's vertices, m = range_margin; an    */
/* image without vertices or neighbours: an empty list and 0 0.              */
/* ------------------------------------------------------------------------ */
typedef struct sfm_depth_views_opts {
    double opt_angle;        /* 10 degrees                                     */
    double min_angle;        /* 3 degrees                                      */
    double max_scale;        /* 1.6                                            */
    double range_margin;     /* 0.25                                           */
    int32_t min_shared;      /* 10                                             */
    int32_t max_neighbors;   /* 4; at most 8                                   */
} sfm_depth_views_opts;
/* [cpu] */
void sfm_depth_views_default_options(sfm_depth_views_opts* opts);
/* [cpu] The arrays are sfm_dense_scene_fetch's.  nb_off[n_images + 1];
 * nb_view and nb_score hold n_images * max_neighbors entries; drange
 * [2 * n_images].  O(views * track length) on the host. */
int sfm_depth_views_select(int32_t n_platforms, int32_t n_images, int64_t n_vertices, const double* K,
                           const int32_t* image_platform, const double* R, const double* C, const float* vert_X,
                           const int64_t* vert_off, const uint32_t* vert_view, const sfm_depth_views_opts* opts,
                           int64_t* nb_off, int32_t* nb_view, double* nb_score, float* drange);

typedef struct sfm_depthmap_opts {
    int32_t half_window;     /* r: 3; 1..5                                     */
    int32_t iterations;      /* 3; 0..16 (0: the initial planes' costs only)   */
    int32_t n_best;          /* 2; at least 1                                  */
    int32_t reserved;
    uint64_t seed;
    int64_t device_bytes;    /* budget for the resident images and maps;
                                0: the library's default, 4 GiB               */
} sfm_depthmap_opts;
/* [cpu] */
void sfm_depthmap_default_options(sfm_depthmap_opts* opts);
typedef struct sfm_depthmap_stats {
    int64_t n_images;        /* active images                                  */
    int64_t n_estimated;     /* estimated pixels of those                      */
    int64_t n_invalid;       /* of those, left at cost 2                       */
    int64_t resident_bytes;  /* gray images, maps, views and pairs             */
    double seconds[3];       /* upload, kernels, download (HIP events).  Host
                                twin: 0, the estimation's wall time, 0.        */
} sfm_depthmap_stats;
/* Every check runs on the host before any device call.  SFM_ERR_INVALID_ARG
 * with a message: a non-positive size, channels other than 1 or 3 on a loaded
 * image, a neighbour index out of range or equal to the image itself, more
 * than 8 neighbours, drange not 0 < d_min < d_max on an image with neighbours,
 * a non-finite camera or a singular K, half_window outside 1..5, iterations
 * outside 0..16, n_best < 1, only one of init_depth / init_normal.
 * SFM_ERR_UNSUPPORTED: the resident set exceeds device_bytes (streaming is not
 * built; the host twin refuses the same calls), an image of 2^31 or more
 * pixels.  init_depth / init_normal (both or neither; laid out as depth /
 * normal, and may be them) replace the random initial planes.  opts NULL = the
 * defaults; stats may be NULL. */
int sfm_depthmap(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                 const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                 const int32_t* nb_view, const float* drange, const float* init_depth, const float* init_normal,
                 const sfm_depthmap_opts* opts, float* depth, float* normal, float* cost, sfm_depthmap_stats* stats);
/* [cpu] the host twin (threads over rows, pass after pass): the same bytes and counts */
int sfm_depthmap_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                      const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                      const int32_t* nb_view, const float* drange, const float* init_depth, const float* init_normal,
                      const sfm_depthmap_opts* opts, float* depth, float* normal, float* cost,
                      sfm_depthmap_stats* stats);

/* The consistency filter.  It reads the unfiltered maps of all images, so the
 * result does not depend on any order.  A pixel p with depth d > 0 and
 * cost <= max_cost is a candidate.  For each neighbour j, in float:
 * h = d * (A [p 1]) + b, z = h2, x = floorf(h0 / z + 0.5f), y likewise (the
 * pixel rounded half up); j agrees when z > 0, 0 <= x <= w_j - 1,
 * 0 <= y <= h_j - 1, depth_j(x, y) > 0 and |z - depth_j| <= rel_tol * z.  The
 * candidate is kept when at least min(min_consistent, n_nb) neighbours agree.
 * depth_out: the depth, or 0; n_agree: the agreeing neighbours of a candidate,
 * else 0; counts[2 i ..] (may be NULL): candidates and kept pixels of image i.
 * The checks on sizes, cameras and neighbours are sfm_depthmap's. */
typedef struct sfm_depthmap_filter_opts {
    float max_cost;          /* 0.5                                            */
    float rel_tol;           /* 0.01                                           */
    int32_t min_consistent;  /* 2                                              */
    int32_t reserved;
} sfm_depthmap_filter_opts;
/* [cpu] */
void sfm_depthmap_filter_default_options(sfm_depthmap_filter_opts* opts);
typedef struct sfm_depthmap_filter_stats {
    int64_t n_candidates, n_kept;
    double seconds[3];       /* as sfm_depthmap_stats                          */
} sfm_depthmap_filter_stats;
int sfm_depthmap_filter(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const double* K, const double* R,
                        const double* C, const int64_t* nb_off, const int32_t* nb_view, const float* depth,
                        const float* cost, const sfm_depthmap_filter_opts* opts, float* depth_out, uint8_t* n_agree,
                        int64_t* counts, sfm_depthmap_filter_stats* stats);
/* [cpu] the host twin: the same bytes and counts */
int sfm_depthmap_filter_host(int32_t n_img, const int32_t* wh, const double* K, const double* R, const double* C,
                             const int64_t* nb_off, const int32_t* nb_view, const float* depth, const float* cost,
                             const sfm_depthmap_filter_opts* opts, float* depth_out, uint8_t* n_agree,
                             int64_t* counts, sfm_depthmap_filter_stats* stats);

/* ------------------------------------------------------------------------ */
/* Dense fusion                                              */
/* The second half of DensifyPointCloud: the filtered depth maps of all      */
/* images become one cloud of points with normals, colours and view lists.   */
/* OpenMVS's FuseDepthMaps walks the images in order and invalidates merged  */
/* pixels as it goes, so its result depends on that order.  This is an       */
/* order-free restatement: a pixel's fate depends on the input maps only,    */
/* never on what another pixel decided, so the device, the host twin and a   */
/* restatement give the same bytes.  Nothing is pinned to OpenMVS's numbers; */
/* this comment is the contract.                                             */
/*                                                                          */
/* Inputs: n_img, wh, K, R, C, nb_off, nb_view as sfm_depthmap_filter takes  */
/* them; depth[n_map] (the filter's depth_out), normal[3 n_map]              */
/* (sfm_depthmap's, camera frame); optionally the colour pool channels,      */
/* img_off, pixels laid out as sfm_undistort's `out`.  pixels NULL: no       */
/* colours (rgb is not written) and every image counts as loaded.  pixels    */
/* given: an image with img_off < 0 counts as all-zero depth.                */
/*                                                                          */
/* Fusion pair list of image i (host): its own nb_view entries in order,     */
/* then, ascending, every image j that lists i as a neighbour and is not yet */
/* in the list; at most 32 entries, later ones are dropped and counted in    */
/* n_pairs_dropped.  A and b of a pair (i, j) are sfm_depthmap's: in double, */
/* rounded once.  Ki = K^-1, R and C are rounded from double once.           */
/*                                                                          */
/* Float arithmetic as in "Dense depth maps": single IEEE operations in the  */
/* order written, dot(a, b) = (a0 b0 + a1 b1) + a2 b2, M [x y 1] has the     */
/* rows (M0 x + M1 y) + M2.  For a vector v in the camera frame of image i,  */
/* R' v has the components (R[c] v0 + R[3+c] v1) + R[6+c] v2, c = 0 1 2      */
/* (R row-major).  World normal of a pixel: N = R' n.  World point of pixel  */
/* p at depth d: Xw = R' (d * (Ki [p 1])) (+) C, d times each component.     */
/* Agreement of pixel p = (x, y) of image i with depth d > 0 against pair j  */
/* (the filter's arithmetic, against the map given): h = d * (A [p 1]) + b,  */
/* z = h2, q = (floorf(h0 / z + 0.5f), floorf(h1 / z + 0.5f)); j agrees when */
/* z > 0, q is inside j, depth_j(q) > 0 and |z - depth_j(q)| <= rel_tol * z  */
/* and, when min_normal_cos > -1, dot(N_i(p), N_j(q)) >= min_normal_cos.     */
/* Fate of a pixel with d > 0: suppressed when some agreeing pair has an     */
/* image index j < i, otherwise emitted; a pixel with d <= 0 (or NaN) is     */
/* neither.  The lowest agreeing index strictly descends along a chain of    */
/* suppressed pixels, so every one of them leads to an emitted pixel.        */
/* A fused point: the contributors are the emitted pixel itself, then its    */
/* agreeing pairs in list order, each with its own pixel q and its own depth */
/* depth_j(q); m of them.  X = the component sums of their world points in   */
/* contributor order, divided by (float)m.  N = the sum of their world       */
/* normals divided by its length sqrtf((s0 s0 + s1 s1) + s2 s2); when        */
/* !(len > 0), the pixel's own world normal.  rgb per channel: the integer   */
/* sum s of the contributors' bytes at their pixels (a 1-channel image       */
/* replicated), then (2 s + m) / (2 m) in integers.  n_views = m;            */
/* view_mask bit k: pair k of the list agrees; src_image = i;                */
/* src_pixel = y w + x.  The cloud is in ascending (image, y, x) order of    */
/* the emitting pixels; that order is part of the contract.                  */
/* ------------------------------------------------------------------------ */
typedef struct sfm_depthmap_fuse_opts {
    float rel_tol;           /* 0.01                                           */
    float min_normal_cos;    /* -1: the normal test is off (PatchMatch normals
                                after three iterations are noisy; DESIGN.md
                                §5l has the measurement)                       */
    int64_t device_bytes;    /* budget for the resident maps, masks and colour
                                pool; 0: the library's default, 4 GiB         */
} sfm_depthmap_fuse_opts;
/* [cpu] */
void sfm_depthmap_fuse_default_options(sfm_depthmap_fuse_opts* opts);
typedef struct sfm_depthmap_fuse_stats {
    int64_t n_points;        /* emitted pixels: the points of the cloud        */
    int64_t n_suppressed;
    int64_t n_pairs_dropped; /* fusion pairs beyond 32 of an image             */
    int64_t resident_bytes;  /* depth, normal, mask and fate of every pixel,
                                the colour bytes, views, pairs, block tables
                                (the cloud itself is not counted)              */
    double seconds[3];       /* upload, kernels, download (HIP events).  Host
                                twin: 0, the fusion's wall time, 0.            */
} sfm_depthmap_fuse_stats;
/* The checks are sfm_depthmap_filter's (sizes, cameras, neighbours), plus:
 * rel_tol negative or not a number, min_normal_cos not a number or above 1,
 * negative device_bytes, negative cap_points, null depth / normal / X, channels
 * other than 1 or 3 on a loaded image: SFM_ERR_INVALID_ARG; the resident set
 * exceeds device_bytes: SFM_ERR_UNSUPPORTED (the host twin refuses the same
 * calls).  They run on the host before any device call.  X[3 cap_points];
 * N[3 cap_points], rgb[3 cap_points], n_views, view_mask, src_image,
 * src_pixel [cap_points] may each be NULL.  When the cloud needs more than
 * cap_points points nothing is written, stats.n_points holds the need and the
 * call returns SFM_ERR_INVALID_ARG with a message; the count of pixels with
 * depth > 0 is always enough.  opts NULL = the defaults; stats may be NULL. */
int sfm_depthmap_fuse(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                      const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                      const int32_t* nb_view, const float* depth, const float* normal,
                      const sfm_depthmap_fuse_opts* opts, int64_t cap_points, float* X, float* N, uint8_t* rgb,
                      uint8_t* n_views, uint32_t* view_mask, int32_t* src_image, int32_t* src_pixel,
                      sfm_depthmap_fuse_stats* stats);
/* [cpu] the host twin (threads over rows): the same bytes and counts */
int sfm_depthmap_fuse_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                           const uint8_t* pixels, const double* K, const double* R, const double* C,
                           const int64_t* nb_off, const int32_t* nb_view, const float* depth, const float* normal,
                           const sfm_depthmap_fuse_opts* opts, int64_t cap_points, float* X, float* N, uint8_t* rgb,
                           uint8_t* n_views, uint32_t* view_mask, int32_t* src_image, int32_t* src_pixel,
                           sfm_depthmap_fuse_stats* stats);
/* [cpu] The view lists of a cloud as a CSR: point k sees view_idx[view_off[k]
 * .. view_off[k + 1]): its own image first, then the images of the set bits of
 * its view_mask in fusion-pair-list order.  view_off[n_points + 1];
 * view_idx NULL: only view_off is filled (to size view_idx). */
int sfm_dense_cloud_views(int32_t n_img, const int64_t* nb_off, const int32_t* nb_view, int64_t n_points,
                          const int32_t* src_image, const uint32_t* view_mask, int64_t* view_off, int32_t* view_idx);
/* [cpu] "ply / format binary_little_endian 1.0 / element vertex n", float
 * x y z, then float nx ny nz when N is given, then uchar red green blue when
 * rgb is given. */
int sfm_dense_cloud_write_ply(const char* path, int64_t n_points, const float* X, const float* N, const uint8_t* rgb);

/* Depth maps, filter and fusion in one call over one set of device buffers:
 * the images are uploaded once and no map crosses the bus unless it is asked
 * for.  The outputs equal, byte for byte, those of sfm_depthmap, then
 * sfm_depthmap_filter over its depth and cost, then sfm_depthmap_fuse over the
 * filter's depth_out and sfm_depthmap's normal with the same colour pool.  The
 * checks are those three calls' (on the host, before any device call).  depth,
 * normal, cost, depth_filtered, n_agree (laid out as the maps) and
 * counts[2 n_img] are each downloaded only when non-NULL.  n_map points are
 * always enough for cap_points. */
typedef struct sfm_densify_stats {
    sfm_depthmap_stats depthmap;          /* the counts; seconds are 0 on the device */
    sfm_depthmap_filter_stats filter;     /* likewise                                */
    sfm_depthmap_fuse_stats fuse;         /* likewise                                */
    double seconds[3];       /* upload, everything up to the last kernel (with
                                the one read-back of the point count),
                                download.  Host twin: the three calls' own
                                seconds stay in their stats; here 0, their
                                sum, 0.                                        */
} sfm_densify_stats;
int sfm_densify(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                const int32_t* nb_view, const float* drange, const float* init_depth, const float* init_normal,
                const sfm_depthmap_opts* opts, const sfm_depthmap_filter_opts* filter_opts,
                const sfm_depthmap_fuse_opts* fuse_opts, int64_t cap_points, float* X, float* N, uint8_t* rgb,
                uint8_t* n_views, uint32_t* view_mask, int32_t* src_image, int32_t* src_pixel, float* depth,
                float* normal, float* cost, float* depth_filtered, uint8_t* n_agree, int64_t* counts,
                sfm_densify_stats* stats);
/* [cpu] the three host twins chained */
int sfm_densify_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                     const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                     const int32_t* nb_view, const float* drange, const float* init_depth, const float* init_normal,
                     const sfm_depthmap_opts* opts, const sfm_depthmap_filter_opts* filter_opts,
                     const sfm_depthmap_fuse_opts* fuse_opts, int64_t cap_points, float* X, float* N, uint8_t* rgb,
                     uint8_t* n_views, uint32_t* view_mask, int32_t* src_image, int32_t* src_pixel, float* depth,
                     float* normal, float* cost, float* depth_filtered, uint8_t* n_agree, int64_t* counts,
                     sfm_densify_stats* stats);

/* ------------------------------------------------------------------------ */
/* Mesh                                                      */
/* The first step of meshWork(): a surface from the filtered depth maps.     */
/* OpenMVS's ReconstructMesh is a Delaunay tetrahedralisation with a graph   */
/* cut: serial and order dependent.  This is a method without an order: the  */
/* depth maps are integrated into a truncated signed distance volume (TSDF), */
/* one lattice point at a time, and the zero level set is extracted by       */
/* marching tetrahedra over the Kuhn split of every cell, with the vertices  */
/* and triangles placed by prefix sums.  The device, the host twin and a     */
/* restatement give the same bytes.  Nothing is pinned to OpenMVS's numbers; */
/* this comment is the contract.                                             */
/*                                                                          */
/* Float arithmetic as in "Dense depth maps": single IEEE operations in the  */
/* order written, dot(a, b) = (a0 b0 + a1 b1) + a2 b2, M q has the rows      */
/* dot(M_row, q).                                                            */
/*                                                                          */
/* Grid: origin[3], voxel > 0, dims = (nx, ny, nz), each >= 1.  Lattice      */
/* point (i, j, k) has the raster index (k ny + j) nx + i and the position   */
/* origin_c + (float)i_c * voxel per component.  nx ny nz >= 2^31, ny above  */
/* 262140 or nz above 65535: SFM_ERR_UNSUPPORTED.                            */
/*                                                                          */
/* Integration.  Inputs n_img, wh, channels, img_off, pixels, K, R, C and    */
/* depth[n_map] as sfm_depthmap_fuse takes them (no neighbour lists, no      */
/* normals): pixels NULL: no colours, every image has a depth map; pixels    */
/* given: an image with img_off < 0 has none.  Per image the host works out  */
/* M = K R in double and rounds once; C is rounded once.  trunc is the       */
/* option, or 3.0f * voxel (in float) when it is 0.  A lattice point X takes */
/* the images that have a depth map in ascending index order:                */
/*   q = X - C, h = M q, z = h2; skip the image unless z > 0;                */
/*   x = floorf(h0 / z + 0.5f), y = floorf(h1 / z + 0.5f); skip unless       */
/*   0 <= x <= w - 1 and 0 <= y <= h - 1;  d = depth(x, y); skip unless      */
/*   d > 0;  sd = d - z; skip when sd < -trunc;                              */
/*   t = (sd < trunc ? sd : trunc) / trunc;  sum = sum + t;  count += 1;     */
/*   with colours, when fabsf(sd) <= trunc: the pixel's bytes are added to   */
/*   three integer sums s (a 1-channel image replicated) and m += 1.         */
/* tsdf = sum / (float)count, or 0 when count is 0; weight = min(count,      */
/* 255); rgb = (2 s + m) / (2 m) per channel in integers, 0 0 0 when m is 0; */
/* has_rgb = (m > 0).  Limit: the depth is sampled at the nearest pixel, as  */
/* the filter and the fusion do; there is no bilinear sampling.              */
/*                                                                          */
/* Extraction.  A lattice point is observed when weight >= min_weight; an    */
/* observed point is inside when tsdf < 0.  Cell (i, j, k) (i < nx - 1, ..)  */
/* is live when its 8 corners are observed.  A lattice point owns the 7      */
/* edges to + (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), slots */
/* 0 to 6.  An owned edge carries a vertex when both ends are observed,      */
/* exactly one end is inside and at least one live cell has both ends among  */
/* its corners; so no vertex is unreferenced.  Vertices come in ascending    */
/* (raster index of the owner, slot) order.  The vertex of edge a -> b       */
/* (owner a): u = ta / (ta - tb), then Xa + u * (Xb - Xa) per component.     */
/* Its colour is a's when u < 0.5f, else b's; when that end has no colour    */
/* (has_rgb 0), the other end's; when neither has, 0 0 0.                    */
/* Live cells are taken in raster order, each split into six tetrahedra      */
/* along the axis permutations xyz, xzy, yxz, yzx, zxy, zyx: permutation     */
/* (p1, p2, p3) gives the corners c0 = (0,0,0), c1 = e_p1, c2 = c1 + e_p2,   */
/* c3 = (1,1,1).  v(n m) is the vertex on the edge between corners n and m.  */
/* By the number of inside corners: 0 or 4: nothing.  One corner a differs   */
/* from the other three b < c < d (corner order): the triangle (v(a b),      */
/* v(a c), v(a d)).  Two inside a1 < a2 and two outside b1 < b2: q0 =        */
/* v(a1 b1), q1 = v(a1 b2), q2 = v(a2 b2), q3 = v(a2 b1) and the triangles   */
/* (q0, q1, q2), (q0, q2, q3).  The second and third vertex of a triangle    */
/* (A, B, C) are swapped when needed so that, with every crossing put at its */
/* edge's midpoint, (B - A) x (C - A) has a positive dot product with (mean  */
/* of the outside corners - mean of the inside corners); that product is a   */
/* non-zero multiple of the tetrahedron's volume in every case, so the rule  */
/* fixes a 6 x 16 table.  Triangles are int32 vertex indices in (cell        */
/* raster, tetrahedron, triangle) order; that order and the vertices' are    */
/* part of the contract.  More than 2^31 - 1 vertices: SFM_ERR_UNSUPPORTED.  */
/* Limit: a sample with tsdf == 0 counts as outside, so the edges that end   */
/* in it give vertices that coincide (up to rounding) and triangles without  */
/* area; n_degenerate counts the triangles of which two vertices lie on      */
/* edges that end in the same corner with tsdf == 0.                         */
/* ------------------------------------------------------------------------ */
typedef struct sfm_mesh_grid {
    float origin[3];
    float voxel;
    int32_t dims[3];         /* nx ny nz                                       */
    int32_t pad;
} sfm_mesh_grid;
/* [cpu] The grid around a cloud, in double: lo / hi = the bounding box of
 * X[3 n_points], voxel_d = (the longest side) / resolution, voxel =
 * (float)voxel_d, origin_c = (float)(lo_c - margin_voxels * voxel_d), dims_c =
 * floor((hi_c - lo_c) / voxel_d) + 2 + 2 margin_voxels.  n_points < 1,
 * resolution < 1, margin_voxels < 0, a coordinate that is not finite or a
 * cloud without extent: SFM_ERR_INVALID_ARG; the grid's limits above:
 * SFM_ERR_UNSUPPORTED. */
int sfm_mesh_grid_fit(int64_t n_points, const float* X, int32_t resolution, int32_t margin_voxels, sfm_mesh_grid* grid);

typedef struct sfm_tsdf_opts {
    float trunc;             /* world units; 0: 3 * voxel                      */
    int32_t pad;
    int64_t device_bytes;    /* budget for the resident maps, colours and
                                volume; 0: the library's default, 4 GiB       */
} sfm_tsdf_opts;
/* [cpu] */
void sfm_tsdf_default_options(sfm_tsdf_opts* opts);
typedef struct sfm_tsdf_stats {
    int64_t n_observed;      /* lattice points with weight > 0                 */
    int64_t resident_bytes;  /* the depth maps, the colour bytes, the views, 9
                                bytes a lattice point and the block counts     */
    double seconds[3];       /* upload, kernels, download (HIP events).  Host
                                twin: 0, the wall time, 0.                     */
} sfm_tsdf_stats;
/* tsdf[n], weight[n], rgb[3 n], has_rgb[n] over the n = nx ny nz lattice
 * points in raster order; rgb and has_rgb are written only when pixels is
 * given and may be NULL otherwise.  Checks (on the host, before any device
 * call; the host twin refuses the same calls): negative n_img, a null
 * argument, a non-positive image size, a camera that is not finite, channels
 * other than 1 or 3 on an image with colours, a voxel that is not positive and
 * finite, an origin that is not finite, a dimension below 1, trunc negative or
 * not a number, negative device_bytes: SFM_ERR_INVALID_ARG; the grid's limits,
 * an image of 2^31 pixels or more, a resident set beyond device_bytes:
 * SFM_ERR_UNSUPPORTED.  opts NULL = the defaults; stats may be NULL. */
int sfm_tsdf_integrate(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                       const uint8_t* pixels, const double* K, const double* R, const double* C, const float* depth,
                       const sfm_mesh_grid* grid, const sfm_tsdf_opts* opts, float* tsdf, uint8_t* weight, uint8_t* rgb,
                       uint8_t* has_rgb, sfm_tsdf_stats* stats);
/* [cpu] the host twin (threads over rows): the same bytes and counts */
int sfm_tsdf_integrate_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                            const uint8_t* pixels, const double* K, const double* R, const double* C, const float* depth,
                            const sfm_mesh_grid* grid, const sfm_tsdf_opts* opts, float* tsdf, uint8_t* weight,
                            uint8_t* rgb, uint8_t* has_rgb, sfm_tsdf_stats* stats);

typedef struct sfm_mesh_opts {
    int32_t min_weight;      /* 1 .. 255; default 1                            */
    int32_t pad;
} sfm_mesh_opts;
/* [cpu] */
void sfm_mesh_default_options(sfm_mesh_opts* opts);
typedef struct sfm_mesh_stats {
    int64_t n_vertices;
    int64_t n_triangles;
    int64_t n_degenerate;    /* see the limit above                            */
    double seconds[3];       /* upload, kernels (with the one read-back of the
                                totals), download.  Host twin: 0, wall, 0.     */
} sfm_mesh_stats;
/* V[3 cap_vertices], rgb[3 cap_vertices] (written when the volume's rgb and
 * has_rgb are given; may be NULL), tri[3 cap_triangles].  The caps behave as
 * cap_points does in the fusion: when either is too small nothing is written,
 * stats holds both needs and the call returns SFM_ERR_INVALID_ARG with a
 * message.  Checks: the grid's, a null tsdf / weight, rgb without has_rgb,
 * min_weight outside 1 .. 255, a negative cap, a null V or tri with a positive
 * cap: SFM_ERR_INVALID_ARG. */
int sfm_mesh_extract(sfm_ctx* ctx, const sfm_mesh_grid* grid, const float* tsdf, const uint8_t* weight,
                     const uint8_t* rgb, const uint8_t* has_rgb, const sfm_mesh_opts* opts, int64_t cap_vertices,
                     int64_t cap_triangles, float* V, uint8_t* vertex_rgb, int32_t* tri, sfm_mesh_stats* stats);
/* [cpu] the host twin: the same bytes and counts */
int sfm_mesh_extract_host(const sfm_mesh_grid* grid, const float* tsdf, const uint8_t* weight, const uint8_t* rgb,
                          const uint8_t* has_rgb, const sfm_mesh_opts* opts, int64_t cap_vertices, int64_t cap_triangles,
                          float* V, uint8_t* vertex_rgb, int32_t* tri, sfm_mesh_stats* stats);

/* Integration and extraction in one call; the volume stays on the device and
 * tsdf[n] / weight[n] are downloaded only when non-NULL.  The outputs equal,
 * byte for byte, those of sfm_tsdf_integrate, then sfm_mesh_extract over its
 * volume.  The checks are the two calls'. */
typedef struct sfm_mesh_reconstruct_stats {
    sfm_tsdf_stats tsdf;     /* the counts; seconds are 0 on the device        */
    sfm_mesh_stats mesh;     /* likewise                                       */
    double seconds[3];       /* upload, everything up to the last kernel,
                                download.  Host twin: 0, the two calls' sum, 0 */
} sfm_mesh_reconstruct_stats;
int sfm_mesh_reconstruct(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                         const uint8_t* pixels, const double* K, const double* R, const double* C, const float* depth,
                         const sfm_mesh_grid* grid, const sfm_tsdf_opts* tsdf_opts, const sfm_mesh_opts* mesh_opts,
                         int64_t cap_vertices, int64_t cap_triangles, float* V, uint8_t* vertex_rgb, int32_t* tri,
                         float* tsdf, uint8_t* weight, sfm_mesh_reconstruct_stats* stats);
/* [cpu] the two host twins chained */
int sfm_mesh_reconstruct_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                              const uint8_t* pixels, const double* K, const double* R, const double* C,
                              const float* depth, const sfm_mesh_grid* grid, const sfm_tsdf_opts* tsdf_opts,
                              const sfm_mesh_opts* mesh_opts, int64_t cap_vertices, int64_t cap_triangles, float* V,
                              uint8_t* vertex_rgb, int32_t* tri, float* tsdf, uint8_t* weight,
                              sfm_mesh_reconstruct_stats* stats);
/* [cpu] "ply / format binary_little_endian 1.0 / element vertex n", float
 * x y z, then uchar red green blue when rgb is given, then "element face m /
 * property list uchar int vertex_indices": a byte 3 and three int32 a face. */
int sfm_mesh_write_ply(const char* path, int64_t n_vertices, const float* V, const uint8_t* rgb, int64_t n_triangles,
                       const int32_t* tri);

/* ------------------------------------------------------------------------ */
/* Mesh texture                                              */
/* The last step of meshWork(): every face chooses the view that sees it     */
/* best, and a texture atlas is baked from the chosen views.  OpenMVS's      */
/* TextureMesh packs charts and optimises seams serially; this is a method   */
/* without an order: a face's place in the atlas follows from its index, and */
/* every face chooses alone.  The device, the host twin and a restatement    */
/* give the same bytes.  Nothing is pinned to OpenMVS's numbers; this        */
/* comment is the contract.                                                  */
/*                                                                          */
/* Float arithmetic as in "Dense depth maps": single IEEE operations in the  */
/* order written, dot(a, b) = (a0 b0 + a1 b1) + a2 b2, M q has the rows      */
/* dot(M_row, q); M = K R is worked out in double and rounded once, C is     */
/* rounded once.  (float) of an int64 rounds to nearest even.                */
/*                                                                          */
/* Inputs: n_img, wh, channels, img_off, pixels, K, R, C as                  */
/* sfm_tsdf_integrate takes them; an image with img_off < 0 is skipped       */
/* entirely (no occluder pass, no candidate).  sfm_mesh_face_views reads no  */
/* pixel bytes: with pixels NULL every image counts.  The mesh is            */
/* V[3 n_vertices] float, tri[3 n_triangles] int32 and, optionally,          */
/* vertex_rgb[3 n_vertices].  Pixel (px, py) has its centre at the integer   */
/* position.                                                                 */
/*                                                                          */
/* 1. Face views.  The views are taken in ascending index order; a to c run  */
/* per view.                                                                 */
/* a. Per corner X of a face: q = X - C, h = M q, z = h2, x = h0 / z,        */
/*    y = h1 / z.  The face is drawable in the view when its three z > 0 and */
/*    its three |x|, |y| <= 1048576.0f (NaN fails).  Xi = (int64)floorf(x *  */
/*    16.0f + 0.5f), Yi likewise.  A2 = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 -  */
/*    Y0).  A2 == 0: the face covers nothing.  A2 < 0: corners 1 and 2 are   */
/*    exchanged, with their z, for b and c, and A2 stands for -A2.           */
/* b. Edge k runs from corner a = (k + 1) % 3 to b = (k + 2) % 3; E_k(P) =   */
/*    (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa) at P = (16 px, 16 py), in      */
/*    int64.  A pixel is covered when for every k: E_k > 0, or E_k == 0 and  */
/*    (Yb - Ya > 0, or Yb - Ya == 0 and Xb - Xa > 0).  So a pixel centre on  */
/*    an edge that two faces share belongs to exactly one of them.  Only     */
/*    pixels of the image count (the walk is over the bounding box, integer  */
/*    ceiling of min / 16 to integer floor of max / 16, clipped).            */
/* c. Every drawable face occludes, whichever way it looks.  Per covered     */
/*    pixel: w_k = 1.0f / z_k, num = ((float)E0 * w0 + (float)E1 * w1) +     */
/*    (float)E2 * w2, d = (float)A2 / num; the pixel keeps the minimum of    */
/*    ((uint64)bits(d) << 32) | face: the nearest face, the lowest index on  */
/*    equal depth, whatever the order of arrival.                            */
/* d. covered(f, v) is the count of b, won(f, v) the number of those pixels  */
/*    that kept f.  f is eligible in v when it is drawable, front-facing     */
/*    (dot((V1 - V0) x (V2 - V0), C - V0) > 0, the cross product's           */
/*    components n0 = e1_1 e2_2 - e1_2 e2_1, n1 = e1_2 e2_0 - e1_0 e2_2,     */
/*    n2 = e1_0 e2_1 - e1_1 e2_0 as written, corners not exchanged), its     */
/*    three unrounded (x, y) lie in [0, w - 1] x [0, h - 1], covered >= 1    */
/*    and won == covered.  face_view[f] is the eligible view with the        */
/*    largest covered, the lowest index on a tie, or -1; face_pixels[f] is   */
/*    that covered, or 0.                                                    */
/* Limits: a face that crosses the camera plane of a view does not occlude   */
/* in it; a face that covers no pixel centre gets the fallback of 2; each    */
/* face chooses alone, there is no seam smoothing.                           */
/*                                                                          */
/* 2. Atlas.  s = cell (4 .. 64), n_sq = (n_triangles + 1) / 2, cols the     */
/* smallest integer with cols cols >= n_sq, rows = ceil(n_sq / cols) (both 0 */
/* without triangles), W = cols s, H = rows s; W or H above 32768:           */
/* SFM_ERR_UNSUPPORTED.  Face f lies in square f / 2, at column (f / 2) %    */
/* cols and row (f / 2) / cols (origin ox = column s, oy = row s), and is    */
/* half f % 2 of it.  Texel (a, b) of a square, 0 <= a, b < s, belongs to    */
/* half 0 when a + b <= s - 2, else to half 1.  Corners 0, 1, 2 in texel     */
/* units from the square's origin (a texel's centre is at + 0.5): half 0:    */
/* (0.5, 0.5) (s - 2.5, 0.5) (0.5, s - 2.5); half 1: (s - 0.5, s - 0.5)      */
/* (2.5, s - 0.5) (s - 0.5, 2.5).  Each half keeps a diagonal of             */
/* extrapolated texels, so a bilinear fetch inside one face's triangle never */
/* reads the other's.  Weights: half 0: l1 = (float)a / (float)(s - 3), l2   */
/* = (float)b / (float)(s - 3); half 1: l1 = (float)(s - 1 - a) / (float)(s  */
/* - 3), l2 = (float)(s - 1 - b) / (float)(s - 3).                           */
/* A texel of a face with face_view = v >= 0: per component P = (V0 + l1 *   */
/* (V1 - V0)) + l2 * (V2 - V0); q = P - C, h = M q, z = h2; unless z > 0 the */
/* texel is fill; x = fminf(fmaxf(h0 / z, 0), w - 1), y likewise; gx =       */
/* floorf(x), dx = x - gx, gx1 = min(gx + 1, w - 1), likewise in y; per      */
/* channel top = p00 + dx * (p10 - p00), bot = p01 + dx * (p11 - p01), val = */
/* top + dy * (bot - top), byte = (uint8_t)floorf(val + 0.5f); a 1-channel   */
/* image is replicated.  A face with face_view -1: with vertex_rgb, per      */
/* channel (c0 + l1 * (c1 - c0)) + l2 * (c2 - c0), clamped to [0, 255] and   */
/* rounded the same way; without, fill.  A texel whose half has no face:     */
/* fill.  texture[3 W H] has its top row first, as a PNM stores it.          */
/* uv[6 n_triangles]: per corner k of face f (the vertex tri[3 f + k]) u =   */
/* ((float)ox + cx) / (float)W, v = 1.0f - ((float)oy + cy) / (float)H.      */
/*                                                                          */
/* Checks, on the host before any device call (the host twins refuse the     */
/* same calls): a null argument, a negative count, a non-positive image      */
/* size, a triangle index outside [0, n_vertices), a face_view outside [-1,  */
/* n_img) or naming a skipped image (or any image when pixels is NULL), a    */
/* coordinate or camera that is not finite, cell outside 4 .. 64, channels   */
/* other than 1 or 3 on a loaded image, negative device_bytes:               */
/* SFM_ERR_INVALID_ARG.  An image of 2^31 pixels or more, n_triangles or     */
/* n_vertices >= 2^31, the atlas's limit, a resident set beyond device_bytes */
/* (the images' bytes where they are sampled, the views, the vertices and    */
/* their colours, the triangles, 12 bytes a face, one identity buffer of 8   */
/* bytes a pixel of the largest image, the texture and the uv):              */
/* SFM_ERR_UNSUPPORTED.  n_triangles == 0 succeeds and writes nothing.       */
/* ------------------------------------------------------------------------ */
typedef struct sfm_mesh_texture_opts {
    int32_t cell;            /* texels along a square's side, 4 .. 64; default 8 */
    uint8_t fill[3];         /* texels without a source; default 0 0 0         */
    uint8_t pad;
    int64_t device_bytes;    /* budget for the resident set; 0: 4 GiB          */
} sfm_mesh_texture_opts;
/* [cpu] */
void sfm_mesh_texture_default_options(sfm_mesh_texture_opts* opts);
/* [cpu] W, H and cols of section 2. */
int sfm_mesh_atlas_fit(int64_t n_triangles, int32_t cell, int32_t* W, int32_t* H, int32_t* cols);

typedef struct sfm_mesh_face_views_stats {
    int64_t n_textured;      /* faces with a view                              */
    int64_t n_untextured;
    int64_t n_not_drawable;  /* (face, view) pairs refused by step a           */
    int64_t sum_pixels;      /* the sum of face_pixels: the mean tells a
                                caller which cell to choose                    */
    int64_t resident_bytes;
    double seconds[3];       /* upload, kernels, download (HIP events).  Host
                                twin: 0, the wall time, 0.                     */
} sfm_mesh_face_views_stats;
/* Section 1: face_view[n_triangles], face_pixels[n_triangles].  opts NULL =
 * the defaults; stats may be NULL. */
int sfm_mesh_face_views(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                        const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                        const float* V, int64_t n_triangles, const int32_t* tri, const sfm_mesh_texture_opts* opts,
                        int32_t* face_view, int32_t* face_pixels, sfm_mesh_face_views_stats* stats);
/* [cpu] the host twin (threads over faces, then over rows): the same bytes and counts */
int sfm_mesh_face_views_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                             const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                             const float* V, int64_t n_triangles, const int32_t* tri, const sfm_mesh_texture_opts* opts,
                             int32_t* face_view, int32_t* face_pixels, sfm_mesh_face_views_stats* stats);

typedef struct sfm_mesh_bake_stats {
    int32_t W, H, cols, pad; /* the atlas, as sfm_mesh_atlas_fit gives it      */
    int64_t resident_bytes;
    double seconds[3];
} sfm_mesh_bake_stats;
/* Section 2 with any face_view (the caller's choice, checked): texture[3 W H]
 * and uv[6 n_triangles]; vertex_rgb may be NULL. */
int sfm_mesh_texture_bake(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                          const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                          const float* V, const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri,
                          const int32_t* face_view, const sfm_mesh_texture_opts* opts, uint8_t* texture, float* uv,
                          sfm_mesh_bake_stats* stats);
/* [cpu] the host twin (threads over rows of the atlas) */
int sfm_mesh_texture_bake_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                               const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                               const float* V, const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri,
                               const int32_t* face_view, const sfm_mesh_texture_opts* opts, uint8_t* texture, float* uv,
                               sfm_mesh_bake_stats* stats);

/* Section 1, then section 2, with face_view left on the device; face_view and
 * face_pixels are downloaded only when non-NULL.  The outputs equal, byte for
 * byte, those of the two calls chained.  The checks are the two calls'. */
typedef struct sfm_mesh_texture_stats {
    sfm_mesh_face_views_stats views;   /* the counts; seconds are 0 on the device */
    sfm_mesh_bake_stats bake;          /* likewise                                */
    int64_t resident_bytes;
    double seconds[3];       /* upload, everything up to the last kernel,
                                download.  Host twin: 0, the two calls' sum, 0 */
} sfm_mesh_texture_stats;
int sfm_mesh_texture(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                     const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                     const float* V, const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri,
                     const sfm_mesh_texture_opts* opts, int32_t* face_view, int32_t* face_pixels, uint8_t* texture, float* uv,
                     sfm_mesh_texture_stats* stats);
/* [cpu] the two host twins chained */
int sfm_mesh_texture_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                          const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                          const float* V, const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri,
                          const sfm_mesh_texture_opts* opts, int32_t* face_view, int32_t* face_pixels, uint8_t* texture,
                          float* uv, sfm_mesh_texture_stats* stats);
/* [cpu] "ply / format binary_little_endian 1.0 / comment TextureFile <name> /
 * element vertex n", float x y z, then "element face m / property list uchar
 * int vertex_indices / property list uchar float texcoord": a byte 3 and three
 * int32, then a byte 6 and six floats a face.  The texture itself is written
 * with sfm_undistort_write_pnm (P6); image encoding stays outside the library. */
int sfm_mesh_write_textured_ply(const char* path, const char* texture_name, int64_t n_vertices, const float* V,
                                int64_t n_triangles, const int32_t* tri, const float* uv);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SFMCORE_H */
