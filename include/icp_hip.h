/* =====================================================================================
 * icp_hip.h -- C ABI of the MI355X-native ICP hot path (libicp_hip.so)
 *
 * Drop-in boundary for the linear-ICP inner loop of PetropoulakisPanagiotis/ICP-Variants.
 * The reference has no FFI; its "plugin surface" is three C++ interfaces resolved at compile
 * time.  Each entry point below names the reference interface it replaces (file:line relative
 * to icp-variants/ in the reference).  The C++14 adaptor classes that keep the reference's
 * method names on top of this ABI are in include/icp_hip_adaptor.hpp; INTEGRATION.md shows the
 * few lines a maintainer of the reference adds to switch over.
 *
 * Conventions (identical to the reference's containers, so no conversion is needed):
 *   points / normals : N x 3 fp32, row-major, 12 B per element  == std::vector<Eigen::Vector3f>::data()
 *   colours          : N x 4 uint8 RGBA                          == std::vector<Vector4uc>::data()   (Eigen.h:36)
 *   pose             : 16 fp32, COLUMN-major 4x4                 == Eigen::Matrix4f::data()
 *   intrinsics       : fx, fy, cx, cy of the depth camera        (Matrix3f K: K(0,0),K(1,1),K(0,2),K(1,2))
 *   max_distance     : SQUARED metres                            (NearestNeighbor.h:16-18, ICPOptimizer.h:154)
 * All functions return ICP_OK (0) or an error code; nothing ever spins (the reference's ASSERT
 * hangs in while(1), Eigen.h:9).  Host pointers only; the context owns every device buffer.
 * One host thread per context; contexts are independent (one per GPU / HIP stream).
 * ===================================================================================== */
#ifndef ICP_HIP_H
#define ICP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icp_ctx icp_ctx;

/* struct Match, NearestNeighbor.h:7-10.  idx = -1 => no match. */
typedef struct icp_match_t { int32_t idx; float weight; } icp_match_t;

enum icp_status {
    ICP_OK = 0,
    ICP_ERR_INVALID_ARG = 1,
    ICP_ERR_HIP = 2,                 /* a HIP runtime call failed; see icp_last_error() */
    ICP_ERR_NO_TARGET = 3,           /* "index needs to be build before querying" NearestNeighbor.h:144-147,335-338 */
    ICP_ERR_NO_SOURCE = 4,
    ICP_ERR_NO_CAMERA = 5,           /* "Set camera params before querying"        NearestNeighbor.h:341-344 */
    ICP_ERR_TARGET_SIZE = 6,         /* "Invalid size of target points"            NearestNeighbor.h:346-349 */
    ICP_ERR_COLOR_MISMATCH = 7,      /* 3-D index queried with colours or vice versa NearestNeighbor.h:149-152,240-243 */
    ICP_ERR_NO_CORRESPONDENCES = 8,  /* reference ASSERT (ICPOptimizer.h:668,680,788) -- reported, never a hang */
    ICP_ERR_NO_DEVICE = 9,
    ICP_ERR_COMM = 10                /* RCCL missing or an RCCL call failed; see icp_comm_last_error() */
};

/* enum values mirror the reference */
enum { ICP_METRIC_POINT_TO_POINT = 0, ICP_METRIC_POINT_TO_PLANE = 1, ICP_METRIC_SYMMETRIC = 2,   /* ICPOptimizer.h:46-48,131-136 */
       ICP_METRIC_GICP = 3,          /* extension: Generalized-ICP, plane-to-plane (Segal, Haehnel, Thrun 2009); see icp_gicp_options */
       ICP_METRIC_COLORED = 4 };     /* extension: colored ICP (Park, Zhou, Koltun 2017); see icp_colored_options */
enum { ICP_MATCH_KNN = 0, ICP_MATCH_PROJECTIVE = 1 };                                               /* ICPOptimizer.h:71-78 */
enum { ICP_WEIGHT_CONSTANT = 0, ICP_WEIGHT_DISTANCES = 1, ICP_WEIGHT_NORMALS = 2, ICP_WEIGHT_COLORS = 3 };   /* weighting.h:8 */
enum { ICP_KNN_BRUTE_FORCE = 0, ICP_KNN_LBVH = 1 };   /* both exact: identical (d2, lowest-index) argmin, bit for bit */

/* The setter surface of ICPOptimizer (ICPOptimizer.h:41-95) as one POD. */
typedef struct icp_params {
    int32_t metric;          /* setMetric                     default 0 (ICP_METRIC_*; 3 = GICP, 4 = colored, extensions) */
    int32_t matching;        /* setMatchingMethod             default 0 (k-NN)    */
    int32_t weighting;       /* setWeightingMethod            default 0           */
    int32_t rejection;       /* setRejectionMethod            default 1 (60 deg)  */
    int32_t color_icp;       /* enableColorICP                default 0           */
    int32_t multires;        /* enableMultiResolution         default 0           */
    int32_t n_iterations;    /* setNbOfIterations             default 20          */
    float   max_distance;    /* setMatchingMaxDistance        default 0.0003f, squared metres */
    float   fx, fy, cx, cy;  /* setCameraParamsMatchingMethod (ICPOptimizer.h:80-82) */
    int32_t width, height;
    int32_t knn_backend;     /* ICP_KNN_* (extension; the reference's own index is an approximate, randomised FLANN kd-tree) */
    int32_t selection;       /* setSelectionMethod: 0 SELECT_ALL, 1 RANDOM_SAMPLING (selection.h:9); 2 normal-space sampling
                                (ICP_SELECT_*, an extension: see icp_nss_options)                                            */
    float   selection_proba; /* Bernoulli probability per point and per iteration (selection.h:88-106)                     */
    uint32_t selection_seed; /* the reference seeds std::mt19937 from random_device (selection.h:76-79: not reproducible);
                                here a counter-based hash of (seed, iteration, point index) decides -- see icp_select_hash */
    int32_t knn_incremental; /* 1 (default): BVH k-NN verifies the previous neighbour with an exact distance bound and skips the
                                tree walk when it provably cannot change (bit-identical results); 0: always walk the tree */
    int32_t record_rmse;     /* bit 0: per-iteration RMSE against the convergence reference (ConvergenceMeasure.h:50-66);
                                bit 1: also the benchmark error (m_runBenchmark, ConvergenceMeasure.h:74-78,104-151) */
} icp_params;

/* Per-iteration record (what the reference prints / records each iteration, ICPOptimizer.h:541-631). */
typedef struct icp_iter_stats {
    int32_t n_src;           /* source points matched this iteration (multires level size) */
    int32_t n_valid;         /* correspondences that entered the solve (ICPOptimizer.h:594-610) */
    float   pose[16];        /* estimatedPose after the iteration, column-major */
    float   rmse;            /* RMSE vs convergence reference, or -1 */
    float   benchmark_error; /* Fontana-style benchmark error (ConvergenceMeasure.h:104-151) when record_rmse & 2, or -1 */
    int32_t status;          /* ICP_OK or ICP_ERR_NO_CORRESPONDENCES for this iteration */
} icp_iter_stats;

/* Stage times of the last icp_run, device milliseconds: the TimeMeasure breakdown (TimeMeasure.h:20-26).  Weighting, rejection
 * and system build are one fused kernel here.  A run in the merged form (k-NN on the LBVH backend, point-to-plane: one launch per
 * iteration) takes them from the device's own clock, stamped by the launches themselves: an iteration is its launch's span from the
 * first block's entry to the last block's exit, solve_ms the run's closing launch, total_ms from the first launch's start to the
 * closing launch's end.  Every other run brackets its stages with HIP events on the stream. */
typedef struct icp_timing {
    double match_ms;         /* matchingTime                                   */
    double weight_reject_build_ms;   /* weighingTime + rejectionTime + system build */
    double solve_ms;         /* reduction + linear solve + pose composition    */
    double total_ms;         /* convergenceTime                                 */
    int32_t iterations;
    int32_t sampled_iterations;   /* iterations whose stage times were taken (== iterations unless icp_set_stage_timing(N != 1)) */
} icp_timing;

/* -------- context -------- */
int icp_ctx_create(int device, icp_ctx** out);
/* Same, but all work is enqueued on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int icp_ctx_create_on_stream(int device, void* hip_stream, icp_ctx** out);
int icp_ctx_destroy(icp_ctx* ctx);
const char* icp_last_error(const icp_ctx* ctx);

/* -------- configuration: ICPOptimizer setters, ICPOptimizer.h:41-95 -------- */
int icp_params_default(icp_params* p);                       /* ICPOptimizer ctor defaults, ICPOptimizer.h:29-37 */
int icp_set_params(icp_ctx* ctx, const icp_params* p);
int icp_get_params(const icp_ctx* ctx, icp_params* p);

/* -------- NearestNeighborSearch::buildIndex, NearestNeighbor.h:24,27 (122-141, 209-232, 324-331) --------
 * Uploads the target once per pair (AoS -> SoA on the device).  normals may be NULL when only
 * icp_query_matches is used; rgba may be NULL unless color_icp / colour weighting is on. */
int icp_set_target(icp_ctx* ctx, const float* xyz, const float* normals, const uint8_t* rgba, int32_t n);
/* Source cloud of estimatePose (ICPOptimizer.h:140); resident across iterations. */
int icp_set_source(icp_ctx* ctx, const float* xyz, const float* normals, const uint8_t* rgba, int32_t n);

/* -------- NearestNeighborSearch::queryMatches, NearestNeighbor.h:25,28 --------
 * transformed_xyz are ALREADY transformed query points (exactly the argument the reference passes);
 * rgba != NULL selects the 6-D colour search (the target must have been set with colours). */
int icp_query_matches(icp_ctx* ctx, const float* transformed_xyz, const uint8_t* rgba, int32_t n, icp_match_t* out);

/* -------- single stages on the resident source (parity-test entry points) --------
 * icp_match      : transformPoints (utils.h:106-118) fused with queryMatches; d2_out (optional) = winning
 *                  squared distance (FLT_MAX when no candidate).
 * icp_correspond : + applyWeights (weighting.h:39-99) + pruneCorrespondences (ICPOptimizer.h:157-174) +
 *                  validity filter (ICPOptimizer.h:594-610).  sums_out (optional, 64 doubles) receives the
 *                  reduced accumulators the solver consumes (layout in DESIGN.md), n_valid_out the count. */
int icp_match(icp_ctx* ctx, const float pose[16], icp_match_t* out, float* d2_out);
/* The search exactly as the loop of icp_run runs it (parity-test entry point for the seeded / incremental path, NearestNeighbor.h:81-97
 * semantics): the fused matcher of the k-NN BVH backend is launched once per pose of poses[0 .. n_poses) (column-major, 16 floats
 * each) on the Morton-sorted resident source -- the first launch unseeded, every further one seeded with the previous launch's
 * neighbours and search state (verify-and-skip tiers, shared walks, spread start: whatever knn_incremental and the build enable),
 * i.e. launch j is iteration j of a run whose poses are dictated by the caller, in the form icp_run takes for the configuration:
 * point-to-plane by default = the merged loop's launches (k_knn_bvh_post_ring: launch j > 0 carries a reducer of launch j - 1 in its
 * first blocks, every matcher block reads pose j from its slot of the pose ring); point-to-point, ICP_HIP_MERGE=0 or the non-linear
 * optimiser = one k_knn_bvh_post launch per pose.  A bounded wait of the
 * device that ran out returns ICP_ERR_HIP.  out / d2_out (optional) receive the LAST launch's
 * records in source order: the Match after weighting + rejection (= what icp_correspond returns; with rejection 0 and constant
 * weights the raw {idx, 1} / {-1, 0} of queryMatches) and the winning squared distance (FLT_MAX when there was no candidate).
 * Needs matching = k-NN, knn_backend = LBVH, a metric other than symmetric, normals on both clouds; ICP_ERR_INVALID_ARG otherwise. */
int icp_match_seeded(icp_ctx* ctx, const float* poses, int32_t n_poses, icp_match_t* out, float* d2_out);
int icp_correspond(icp_ctx* ctx, const float pose[16], icp_match_t* out, double* sums_out, int32_t* n_valid_out);

/* -------- one iteration / the whole loop: LinearICPOptimizer::estimatePose, ICPOptimizer.h:493-663 --------
 * pose_inout is the caller-owned in/out initialPose (ICPOptimizer.h:140,538,659).
 * icp_iterate runs stages 2-5 once on the full-resolution source (no multires bookkeeping).
 * icp_run runs n_iterations (or the multi-resolution schedule, ICPOptimizer.h:503-525,634-655) without
 * any host round trip inside the loop; stats (optional) receives up to max_stats records.
 * Degenerate systems (few or badly placed correspondences) are solved by the reference's own rank rules, in fp64:
 *   point-to-plane: singular values <= 6 eps_f32 sigma_max of the 4n x 6 system are dropped (JacobiSVD::solve, ICPOptimizer.h:757-758),
 *     the minimum-norm solution of the rest is taken (an eigenvalue cut at (6 eps_f32)^2 on the normal matrix; the LDL^T fast path is
 *     taken only where that rule provably keeps all six directions); GICP and colored ICP share this solve;
 *   symmetric: FullPivLU's rule, pivots <= 6 eps_f32 |max pivot| are zero and their unknowns 0 (:866-868).  When the rotation part of
 *     the solution is exactly 0 (source on target, one correspondence) the reference divides by tan_theta = 0 (:878-885): the pose of
 *     that iteration is all NaN with status ICP_OK and the true n_valid, and the next iteration reports ICP_ERR_NO_CORRESPONDENCES;
 *   point-to-point: Kabsch with the reflection guard, R = U diag(1, 1, det(U V^T)) V^T (ProcrustesAligner.h:55-64).  A Procrustes matrix
 *     of rank <= 1 leaves a family of optimal rotations, of which this library returns: rank 0 (sigma_1 <= f, f = (3 eps_f32)^2 x the
 *     largest |sum w d_j s_k|: one correspondence, coincident points) R = I, as the reference does; rank 1 (sigma_2 <= max(3 eps_f32
 *     sigma_1, f): two correspondences, a line) the rotation by the smallest angle that takes v_1 to u_1 -- about v_1 x u_1, and for
 *     u_1 = -v_1 the half turn about e_k - (e_k . v_1) v_1 with k the smallest |v_1k|.  Parity unpinned for rank 1: what Eigen's JacobiSVD
 *     returns there cannot be obtained without Eigen. */
int icp_iterate(icp_ctx* ctx, float pose_inout[16], icp_iter_stats* stats);
int icp_run(icp_ctx* ctx, float pose_inout[16], icp_iter_stats* stats, int32_t max_stats, int32_t* n_iterations_run);
int icp_get_timing(const icp_ctx* ctx, icp_timing* out);

/* -------- multi-start ICP (extension: the reference has no counterpart) --------
 * ICP is local: from a poor initial pose it settles in a wrong minimum.  icp_run_multistart aligns the context's pair from
 * n_starts initial poses at once (initial_poses: n_starts x 16 floats, column-major) -- one set of launches per ICP iteration for
 * all starts, the target index, the source levels and the random draws shared.  Start k's trajectory equals icp_run from
 * initial_poses[k] on the same context with the same params, bit for bit: every record of stats[k * max_stats ..] (n_src, n_valid,
 * pose, status; rmse and benchmark_error -1) and results[k].pose.  A start that loses all its correspondences reports it in its own
 * status (ICP_ERR_NO_CORRESPONDENCES, pose left where icp_run leaves it); the call returns ICP_OK unless an argument is invalid or a
 * HIP call fails.  Score of a start, at its final pose, on the FULL-resolution source (no multires level, no random sample): every
 * finite source point moved by the pose (utils.h:113-115) and matched in 3-D against the target's xyz (also with color_icp on) is an
 * inlier when its squared distance is <= max_distance -- exactly when icp_match would return idx >= 0 for it; n_inliers, fitness =
 * n_inliers / finite source points (both exact integers, divided in fp64 and rounded once to fp32; 0 when the source has no finite point:
 * such a source is not refused, every start reports ICP_ERR_NO_CORRESPONDENCES and keeps its pose), inlier_rmse = sqrt(sum d^2 /
 * n_inliers) (fp64 sum in a fixed order, one rounding to fp32), -1 without inliers.
 * *best_out (optional): the start with the most inliers, ties to the smaller inlier_rmse, then to the lower index.
 * Supported: k-NN matching on the LBVH backend (3-D or colour 6-D), every metric, weighting, rejection, multires and selection (the draws
 * of RANDOM_SAMPLING and of normal-space sampling are shared between the starts); 1 <= n_starts <= 256.  NOT supported (ICP_ERR_INVALID_ARG, see icp_last_error): projective matching, the
 * brute-force backend, record_rmse != 0 and the non-linear optimiser.  stats may be NULL; n_iterations_run (optional) receives the
 * iterations of the schedule, the same for every start. */
typedef struct icp_start_result {
    float   pose[16];      /* final pose of this start, column-major */
    int32_t status;        /* what icp_run would have returned for this start alone */
    int32_t n_inliers;     /* full-resolution source points with a 3-D neighbour within max_distance at the final pose */
    float   fitness;       /* n_inliers / finite source points, 0 without a finite source point */
    float   inlier_rmse;   /* sqrt(sum d2 / n_inliers), -1 when n_inliers == 0 */
} icp_start_result;
int icp_run_multistart(icp_ctx* ctx, const float* initial_poses, int32_t n_starts, icp_start_result* results, icp_iter_stats* stats,
                       int32_t max_stats, int32_t* n_iterations_run, int32_t* best_out);
/* The same breakdown iteration by iteration for the last icp_run (what TimeMeasure accumulates, before the sum): entry i is the
 * device time of iteration i in milliseconds, or -1 when that iteration was not sampled (icp_set_stage_timing(N != 1)).  Any of
 * the three arrays may be NULL; *count_out = iterations of the last run. */
int icp_get_iteration_times(const icp_ctx* ctx, float* match_ms, float* weight_reject_build_ms, float* solve_ms, int32_t max_out, int32_t* count_out);
/* How icp_run fills the stage breakdown: 0 = whole-run time only, 1 = every iteration (default; what TimeMeasure does),
 * N > 1 = every Nth iteration (rotating offset), stage sums scaled by iterations / sampled.
 * The merged form reads the device's clock inside its launches: no stream cost, the mode only selects what is reported.  The
 * other forms bracket with HIP events at about 4 us of stream time each, i.e. mode 1 is ~10 % of a 0.07 ms iteration there. */
int icp_set_stage_timing(icp_ctx* ctx, int32_t every_nth);
/* The iteration schedule icp_run will execute (pure host logic, no device needed): one decimation factor per
 * iteration, 0 = full cloud without selection.  ICPOptimizer.h:503-516,540,634-655 / PointCloud.h:325-343. */
int icp_schedule(const icp_params* p, int32_t n_src, int32_t* factors_out, int32_t max_out, int32_t* count_out);

/* -------- the non-linear optimiser: CeresICPOptimizer (ICPOptimizer.h:181-483), selected per context --------
 * With it selected, icp_run / icp_iterate / icp_track_depth_frames / icp_batch_run keep the linear path's loop (schedule, selection,
 * matching, weighting, rejection) and replace its solve by one Levenberg-Marquardt minimisation per ICP iteration over the residual
 * blocks of constraints.h, from x = 0 (angle-axis rotation, translation), composed from the left: estimatedPose = T(x) * estimatedPose.
 * The options are those of configureSolver (ICPOptimizer.h:352-360) and otherwise Ceres' defaults; DESIGN.md gives the contract.
 * Iterations whose solve finds no residual block report ICP_ERR_NO_CORRESPONDENCES with the pose unchanged, like the linear path. */
typedef struct icp_lm_options {
    double initial_trust_region_radius;    /* 1e4   */
    double max_trust_region_radius;        /* 1e16  */
    double min_trust_region_radius;        /* 1e-32 */
    double min_relative_decrease;          /* 1e-3  */
    double min_lm_diagonal;                /* 1e-6  */
    double max_lm_diagonal;                /* 1e32  */
    double function_tolerance;             /* 1e-6  */
    double gradient_tolerance;             /* 1e-10 */
    double parameter_tolerance;            /* 1e-8  */
    int32_t max_num_iterations;            /* 10 (configureSolver); 0 .. 1000 */
    int32_t max_num_consecutive_invalid_steps;   /* 5 (>= 1) */
    int32_t jacobi_scaling;                /* 1 */
} icp_lm_options;
enum { ICP_LM_CONVERGENCE = 0, ICP_LM_NO_CONVERGENCE = 1, ICP_LM_FAILURE = 2, ICP_LM_NO_RESIDUALS = 3 };   /* ceres::TerminationType + the empty problem */
/* One record per ICP iteration of the last run (Solver::Summary). */
typedef struct icp_lm_summary {
    int32_t iterations;          /* LM iterations after iteration 0 (the index of the last one) */
    int32_t successful_steps;    /* Ceres' count: iteration 0 included */
    int32_t unsuccessful_steps;  /* rejected and invalid steps that completed an iteration */
    int32_t invalid_steps;       /* steps the damped system or the model change refused */
    int32_t termination;         /* ICP_LM_* */
    int32_t n_residual_blocks;
    uint32_t accepted_steps_mask;  /* bit k - 1: LM iteration k (1 .. 32) took its step (accepted) */
    uint32_t invalid_steps_mask;   /* bit k - 1: LM iteration k had an invalid step; the other iterations < `iterations` were rejected,
                                      and iteration `iterations` ended the solve on a tolerance when its bit is in neither mask */
    double initial_cost, final_cost;     /* 1/2 sum r^2 at x = 0 and at the final x */
    double trust_region_radius;          /* at termination */
    double x[6];                         /* the increment composed into the pose (0 after ICP_LM_FAILURE) */
} icp_lm_summary;
int icp_lm_options_default(icp_lm_options* opt);
/* opt != NULL selects the non-linear optimiser with these options (copied), NULL returns to the linear one. */
int icp_set_optimizer(icp_ctx* ctx, const icp_lm_options* opt);
/* The records of the last run through the non-linear optimiser: out[0 .. min(max, count)), *count = ICP iterations of that run. */
int icp_get_lm_summaries(const icp_ctx* ctx, icp_lm_summary* out, int32_t max, int32_t* count);

/* -------- Generalized-ICP, plane-to-plane (extension: the reference has no counterpart), params.metric = ICP_METRIC_GICP --------
 * Every point carries the covariance C = I - (1 - epsilon) n n^T of a plane with unit normal n (= V diag(epsilon, 1, 1) V^T).
 * GICP normal of a point, computed once per cloud on the full-resolution cloud and cached (every call that replaces a cloud, and
 * icp_set_gicp_options, drops the cache; multires levels and random samples read the normal of their original point):
 *   covariance_k = k > 0: the k smallest (fp32 d^2, index) pairs over the cloud's finite points (the point itself included), fp64 mean
 *     and covariance, fp64 Jacobi; the eigenvector of the smallest eigenvalue rounded once to fp32, no viewpoint flip.  A non-finite
 *     point, or a cloud with fewer than 3 finite points: NaN; fewer than k finite points: all of them; zero covariance: (1, 0, 0).
 *   covariance_k = 0: the cloud's own normals (the loop returns ICP_ERR_INVALID_ARG for a cloud without them).
 * One correspondence (the record after weighting and rejection, as icp_correspond returns it): p = the fp32 transformed source point
 * (icp_transform_points), q = the fp32 target point, r = q - p in fp64; a = the target's GICP normal, b = the source's moved by the pose
 * in fp32 (icp_transform_normals), both normalised in fp64; Sigma = 2I - (1 - epsilon)(a a^T + b b^T) = C_t + R C_s R^T, M = Sigma^-1
 * (adjugate / determinant, fp64); J = [ -[p]x | I ] (x = (alpha, beta, gamma, tx, ty, tz), the point-to-plane linearisation).  The pair
 * enters when the validity filter passes and a, b are finite with non-zero norm: H += w^2 J^T M J, g += w^2 J^T M r, in the sums
 * icp_correspond returns ([0] n, [1..3] sum s, [4..6] sum d, [7..27] upper triangle of H row-major, [28..33] g; fixed-order fp64).
 * Solve: H x = g as point-to-plane's (LDL^T, eigen fallback), then the point-to-plane composition Rx Ry Rz, dT * pose in fp32.
 * Supported: k-NN matching (both backends, 3-D and colour), every weighting, rejection, multires, selection, record_rmse, icp_iterate,
 * icp_run, icp_correspond, icp_batch_run, icp_track_depth_frames.  ICP_ERR_INVALID_ARG at loop start (see icp_last_error): projective
 * matching, the non-linear optimiser, icp_run_multistart, icp_match_seeded. */
typedef struct icp_gicp_options {
    float   epsilon;        /* plane-to-plane regulariser, default 1e-3, 0 < epsilon <= 1 */
    int32_t covariance_k;   /* 20 (default): n from the k-NN PCA of the cloud; 0: n = the cloud's own normals; allowed {0, 5, 10, 20} */
} icp_gicp_options;
int icp_gicp_options_default(icp_gicp_options* opt);
int icp_set_gicp_options(icp_ctx* ctx, const icp_gicp_options* opt);   /* NULL = defaults */
int icp_get_gicp_options(const icp_ctx* ctx, icp_gicp_options* opt);
/* The per-point GICP normals the loop uses, original point order, n x 3 floats (NaN where undefined); computed on demand.
   which: 0 target, 1 source.  out[0 .. min(n, max_points)) is written, *n_out (optional) = n. */
int icp_get_gicp_normals(icp_ctx* ctx, int32_t which, float* out, int32_t max_points, int32_t* n_out);

/* -------- Trimmed ICP and robust kernels (extension: the reference has no counterpart), per context --------
 * Off (kernel = NONE and overlap = 1, the default): nothing changes, every loop form is chosen as without this call.
 * On, per ICP iteration over that iteration's query set (multires level or random sample):
 *   1. weighting, rejection and the validity filter as icp_correspond runs them give each record (idx, w) and the m pairs that enter;
 *   2. r2 = ((e0*e0 + e1*e1) + e2*e2) in fp32, e = s - d (s: the transformed source point, d: the record's target xyz; for every metric
 *      and matcher, colour ICP included); r2 may be +inf, never NaN; residuals are ordered by their uint32 bit pattern;
 *   3. K = clamp(ceil((double)overlap * m), 1, m); t = the K-th smallest r2; a pair with r2 > t is trimmed: its record becomes {-1, w};
 *      ties at t are kept, so M >= K;
 *   4. sigma = (double)options.sigma when > 0, else 1.4826 * sqrt((double)med), med = the ceil(K/2)-th smallest r2;
 *   5. per kept pair, fp64: u = sqrt((double)r2) / sigma, c = (double)tuning (the kernel's standard constant when 0), q = u / c;
 *      HUBER rho = u <= c ? 1 : c / u;  CAUCHY rho = 1 / (1 + q*q);  TUKEY rho = u < c ? (1 - q*q)*(1 - q*q) : 0;  NONE rho = 1;
 *      rho = 1 when sigma is 0 or +inf;
 *   6. point-to-point: w' = (float)((double)w * rho); point-to-plane, symmetric, GICP (rows scaled by w): w' = (float)((double)w * sqrt(rho));
 *   7. the metric's sums and solve as without robust mode, on these records: n_valid = the kept pairs that pass the validity filter
 *      (GICP's own normal filter included); Tukey's rho = 0 pairs stay in with weight 0.
 * m = 0: ICP_ERR_NO_CORRESPONDENCES as today.  Supported: k-NN (both backends, 3-D and colour) and projective matching, every metric,
 * weighting, rejection, multires, selection, record_rmse; icp_iterate, icp_run, icp_correspond (its records and sums are the robust
 * ones), icp_batch_run, icp_track_depth_frames.  ICP_ERR_INVALID_ARG while on: the non-linear optimiser (at loop start),
 * icp_run_multistart, icp_match_seeded. */
enum { ICP_ROBUST_NONE = 0, ICP_ROBUST_HUBER = 1, ICP_ROBUST_CAUCHY = 2, ICP_ROBUST_TUKEY = 3 };
typedef struct icp_robust_options {
    int32_t kernel;    /* ICP_ROBUST_*                                                                  default NONE */
    float   tuning;    /* c; 0 = the kernel's standard constant (1.345 / 2.3849 / 4.6851, as fp32)     default 0 */
    float   sigma;     /* > 0: fixed scale in metres; 0: adaptive, from the median                      default 0 */
    float   overlap;   /* trim ratio xi, 0 < xi <= 1; 1 = no trimming                                   default 1 */
} icp_robust_options;
typedef struct icp_robust_stats {   /* one per ICP iteration of the last call */
    int32_t n_entering;  /* m: pairs that passed weighting, rejection and the validity filter */
    int32_t n_kept;      /* M: pairs kept after trimming (ties at the threshold kept, so M >= K) */
    float   trim_d2;     /* t: the K-th smallest r^2 (-1 when m = 0) */
    float   sigma;       /* the scale used, rounded to fp32; -1 when kernel == NONE or m = 0 */
} icp_robust_stats;
int icp_robust_options_default(icp_robust_options* opt);
/* Validation: kernel in 0..3, tuning and sigma finite and >= 0, 0 < overlap <= 1; else ICP_ERR_INVALID_ARG (reason in icp_last_error). */
int icp_set_robust_options(icp_ctx* ctx, const icp_robust_options* opt);   /* NULL = defaults */
int icp_get_robust_options(const icp_ctx* ctx, icp_robust_options* opt);
/* One record per iteration of the last icp_iterate, icp_run or icp_correspond call on the context (icp_track_depth_frames: the last
 * tracked frame's run; icp_batch_run: each context's own last pair); none when robust mode was off for that call.  Iterations with no
 * work: {0, 0, -1, -1}.  out[0 .. min(max_out, count)), *count_out = the number of records. */
int icp_get_robust_stats(const icp_ctx* ctx, icp_robust_stats* out, int32_t max_out, int32_t* count_out);

/* -------- Normal-space sampling (extension: the reference has SELECT_ALL and RANDOM_SAMPLING only), params.selection = 2 --------
 * Rusinkiewicz and Levoy, "Efficient Variants of the ICP Algorithm" (3DIM 2001): the source points are bucketed by normal direction and
 * sampled uniformly across the buckets, so that the few points on small features survive subsampling beside the big planes.
 * selection_proba and selection_seed keep their meaning; grid and resample are per context (icp_nss_options).
 * Bucket of a source point, from its stored, untransformed fp32 normal (x, y, z), every operation in fp32 with IEEE division:
 *   none when a component of the point or of the normal is non-finite or m = max(|x|, |y|, |z|) is 0; else a = the lowest axis with
 *   |n_a| == m, face = 2a + (n_a < 0), (u, v) = the other two components in axis order, each divided by m,
 *   cell(t) = min(grid - 1, (int)floorf((t + 1.0f) * (0.5f * grid))), bucket = face * grid^2 + cell(v) * grid + cell(u).
 *   (grid is odd so that an axis-aligned normal falls in the middle of a cell, not on a corner.)
 * Draw of iteration i: the base set is RANDOM_SAMPLING's (the iteration's multires level list, or all points for factor 0); its points with
 *   a bucket are the m candidates, cnt_b of them in bucket b.  M = clamp(ceil((double)selection_proba * m), 0, m): proba <= 0 gives an empty
 *   iteration (ICP_ERR_NO_CORRESPONDENCES, as an empty random draw); proba >= 1 gives all CANDIDATES -- unlike RANDOM_SAMPLING's take-all,
 *   which also keeps the points without a usable normal.  Quotas by water-filling: c = the smallest integer with sum_b min(cnt_b, c) >= M,
 *   q_b = min(cnt_b, c); the excess E = sum q_b - M is taken, one each, from the E buckets with cnt_b >= c whose key
 *   icp_select_hash(seed, i, 0x80000000u | b) is smallest.  Bucket b contributes its q_b candidates with the smallest
 *   icp_select_hash(seed, i, original index).  For a fixed (seed, iteration) that hash is a bijection of the index, so keys never tie and
 *   exactly M points are selected.  The list is in increasing original index.
 * resample = 0 (held draws): iteration i uses the draw of the first iteration of the schedule with the same decimation factor, whose index
 *   is the hash's iteration word.  A held draw is a level of its own: on the LBVH backend it is Morton-sorted like a multires level, and the
 *   run takes the seeded (and, for point-to-plane, merged) form a SELECT_ALL run on a cloud of that size takes.
 * Applies wherever RANDOM_SAMPLING does: icp_run, icp_run_multistart (draws shared between the starts), icp_batch_run,
 * icp_track_depth_frames, with every matcher, metric, weighting, rejection, multires, robust mode and the non-linear optimiser;
 * icp_iterate, icp_correspond, icp_match and icp_match_seeded ignore `selection`.  A source without normals: ICP_ERR_INVALID_ARG at loop
 * start (see icp_last_error). */
enum { ICP_SELECT_ALL = 0, ICP_SELECT_RANDOM = 1, ICP_SELECT_NORMAL_SPACE = 2 };
typedef struct icp_nss_options {
    int32_t grid;      /* cells per cube-face edge, {3, 5, 7}, default 5 -> 6*grid^2 buckets (54 / 150 / 294) */
    int32_t resample;  /* 1 (default): a new draw every iteration, like RANDOM_SAMPLING; 0: one draw per level, held for the run */
} icp_nss_options;
int icp_nss_options_default(icp_nss_options* opt);
/* Validation: grid in {3, 5, 7}, resample in {0, 1}; else ICP_ERR_INVALID_ARG (reason in icp_last_error). */
int icp_set_nss_options(icp_ctx* ctx, const icp_nss_options* opt);   /* NULL = defaults */
int icp_get_nss_options(const icp_ctx* ctx, icp_nss_options* opt);
/* The bucket of every source point, original order, 0xFFFF = none; computed on demand, cached per source and grid.
   out[0 .. min(n, max_points)) is written, *n_out (optional) = n. */
int icp_get_normal_buckets(icp_ctx* ctx, uint16_t* out, int32_t max_points, int32_t* n_out);
/* The query set (original source indices, increasing) of iteration `iteration` of the last icp_run / icp_run_multistart / the context's
   last batch pair / last tracked frame, for selection 1 and 2; ICP_ERR_INVALID_ARG when that run had selection 0 or iteration is out of
   range.  Valid until the next call on the context that runs a loop or replaces the source.  out[0 .. min(count, max_out)) is written,
   *n_out (optional) = count. */
int icp_get_selection(icp_ctx* ctx, int32_t iteration, int32_t* out, int32_t max_out, int32_t* n_out);

/* -------- Colored ICP (extension: the reference has no counterpart), params.metric = ICP_METRIC_COLORED --------
 * Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited" (ICCV 2017): point-to-plane plus a photometric term along the
 * target's tangent planes.  Both clouds need colours, the target needs normals.  Intensity of a point: I = (R + G + B) / 765.0 in fp64.
 * Colour gradient of target point i, computed once per target on the device and cached (every call that replaces the target, and
 * icp_set_colored_options, drops the cache): n = i's own normal normalised in fp64; the k smallest (fp32 d^2, index) pairs over the target's
 * finite points (the point itself included), m of them; one row per neighbour j != i, a_j = q'_j - p with q'_j = q_j - n ((q_j - p).n),
 * b_j = I_j - I_i; one constraint row a = (m - 1) n, b = 0; (A^T A) d = A^T b by adjugate and determinant in fp64, d rounded once to fp32.
 * A non-finite point or normal, or a zero normal: NaN; fewer than 3 neighbours or det(A^T A) <= 1e-12 (tr(A^T A) / 3)^3: (0, 0, 0).
 * One correspondence (the record after weighting and rejection, as icp_correspond returns it): p = the fp32 transformed source point,
 * q = the fp32 target point, n = the target normal (unit, fp64), d = its gradient widened to fp64, J = [ -[p]x | I ], lambda = the fp32
 * field widened: j_G = n^T J, r_G = n.(q - p); j_C = d^T (I - n n^T) J, r_C = I_s - I_q - d^T (I - n n^T)(p - q), with
 * I_s - I_q = ((R + G + B)_s - (R + G + B)_q) / 765.0 (one rounding).  The pair enters when the
 * validity filter passes and n, d are finite with |n| > 0: H += w^2 (lambda j_G^T j_G + (1 - lambda) j_C^T j_C),
 * g += w^2 (lambda j_G^T r_G + (1 - lambda) j_C^T r_C), in the sums icp_correspond returns (GICP's layout).  Solve and composition:
 * point-to-plane's.  Supported: k-NN matching (both backends, 3-D and colour), every weighting, rejection, multires, selection,
 * record_rmse, robust mode, icp_iterate, icp_run, icp_correspond, icp_batch_run, icp_track_depth_frames.  ICP_ERR_INVALID_ARG at loop
 * start (see icp_last_error): projective matching, the non-linear optimiser, a cloud without colours, a target without normals; always:
 * icp_run_multistart, icp_match_seeded. */
typedef struct icp_colored_options {
    float   lambda_geometric;   /* weight of the geometric term, 0 <= lambda <= 1, default 0.968 (Park's sigma) */
    int32_t gradient_k;         /* neighbours of a colour gradient, {5, 10, 20}, default 20 */
} icp_colored_options;
int icp_colored_options_default(icp_colored_options* opt);
int icp_set_colored_options(icp_ctx* ctx, const icp_colored_options* opt);   /* NULL = defaults */
int icp_get_colored_options(const icp_ctx* ctx, icp_colored_options* opt);
/* The target's colour gradients the loop uses, original point order, n x 3 floats (NaN where undefined); computed on demand.
   out[0 .. min(n, max_points)) is written, *n_out (optional) = n. */
int icp_get_color_gradients(icp_ctx* ctx, float* out, int32_t max_points, int32_t* n_out);

/* -------- Stopping on a converged pose (extension: the reference always runs its whole schedule), per context --------
 * Off (the default): every loop runs its whole schedule, exactly as without this call.  On: the loop stops, decided on the device, after
 * the first iteration i with streak >= patience and i + 1 >= min_iterations.
 * The measure of iteration i, from two fp32 poses widened to fp64: A = the pose after the iteration, B = the pose it searched at (the
 * incoming pose for iteration 0); dR = R_A R_B^T (each entry (a0 b0 + a1 b1) + a2 b2), dt = t_A - dR t_B;
 *   rotation    = 0.5 * sqrt(((dR21 - dR12)^2 + (dR02 - dR20)^2) + (dR10 - dR01)^2) = |sin theta|; +inf when trace(dR) - 1 <= 0 (> 90 deg);
 *   translation = |dt|;   both rounded once to fp32.
 * The iteration MEETS the criterion when rotation <= rotation_eps && translation <= translation_eps (a NaN fails it).
 * Iteration i is ELIGIBLE when its status is ICP_OK, its decimation factor (icp_schedule) equals that of the schedule's last iteration
 * and, for i > 0, that of iteration i - 1 (coarse multires levels and the first iteration of a new level never count).
 * streak: 0 after an ineligible iteration or an eligible one that misses the criterion, + 1 after an eligible one that meets it.
 * A stopped run: pose_inout = the pose after iteration i, *n_iterations_run = i + 1, records 0 .. i are bit for bit those of the same run
 * with the option off (icp_iter_stats, icp_robust_stats, icp_lm_summary), nothing is reported beyond record i; icp_timing.iterations,
 * icp_get_iteration_times and icp_track_frame.iterations report i + 1; the return status is that of the records reported;
 * icp_get_selection keeps serving the planned draws.  A run that never meets the criterion is the run with the option off.
 * Honoured by icp_run, icp_batch_run (each context's own options) and icp_track_depth_frames, with every matcher, metric, weighting,
 * rejection, multires, selection, robust mode and the non-linear optimiser; icp_iterate, icp_correspond, icp_match and icp_match_seeded
 * ignore it; icp_run_multistart returns ICP_ERR_INVALID_ARG while it is enabled (its starts share their launches). */
typedef struct icp_convergence_options {
    int32_t enabled;          /* 0 (default): every loop runs its whole schedule */
    float   rotation_eps;     /* > 0, finite: bound on the rotation measure (|sin theta|, ~radians)       default 1e-6 */
    float   translation_eps;  /* > 0, finite: bound on the translation measure, metres                     default 1e-6 */
    int32_t min_iterations;   /* >= 1: no stop before this many iterations have run                        default 1 */
    int32_t patience;         /* 1..8: consecutive eligible iterations that must meet both bounds          default 1 */
} icp_convergence_options;
typedef struct icp_convergence_step { float rotation, translation; int32_t eligible, streak; } icp_convergence_step;
typedef struct icp_convergence_result {
    int32_t converged;            /* 1: the last run stopped on the criterion */
    int32_t iterations_run, iterations_planned;
    float   rotation, translation;/* the measure of the last iteration that ran; -1 when the option was off or nothing ran */
} icp_convergence_result;
int icp_convergence_options_default(icp_convergence_options* opt);
/* NULL = defaults (off).  Validation (also while enabled == 0): enabled in {0, 1}, both eps finite and > 0, min_iterations >= 1,
 * patience in 1..8; else ICP_ERR_INVALID_ARG (reason in icp_last_error). */
int icp_set_convergence_options(icp_ctx* ctx, const icp_convergence_options* opt);
int icp_get_convergence_options(const icp_ctx* ctx, icp_convergence_options* opt);
/* The last icp_run on the context (icp_batch_run: the context's own last pair; icp_track_depth_frames: the last tracked frame). */
int icp_get_convergence(const icp_ctx* ctx, icp_convergence_result* out);
/* One step per iteration that ran, of the same run; none when the option was off.  out[0 .. min(max_out, count)), *count_out = count. */
int icp_get_convergence_trace(const icp_ctx* ctx, icp_convergence_step* out, int32_t max_out, int32_t* count_out);

/* -------- Reciprocal (mutual nearest-neighbour) correspondence rejection (extension: the reference has no counterpart), per context --------
 * The "compatibility" test of Rusinkiewicz and Levoy (3DIM 2001), PCL's setUseReciprocalCorrespondences: a pair (s, t) is kept only if s is
 * also the nearest source point to t.  Off (the default): nothing changes, every loop form is chosen as without this call.
 * On, per ICP iteration, behind the matcher and in front of weighting, rejection and the robust chain: every query k of the iteration's
 * query set (multires level or sample) whose raw match idx = t is >= 0 is JUDGED; i = the query's ORIGINAL source index.  The test runs in
 * the source's own frame against the full-resolution resident source, whatever level or sample the iteration runs on (P = the pose the
 * iteration searched at, column-major; every operation one fp32 rounding, no fused contraction):
 *   d   = t_pos - P[12..14]                                  (three subtractions)
 *   q_x = (P[0] d_x + P[1] d_y) + P[2] d_z,  q_y with P[4..6],  q_z with P[8..10]   (the transpose of the 3x3 block applied to d)
 *   d2(j) = (dx dx + dy dy) + dz dz,  dx = q_x - s_j.x, dy = q_y - s_j.y, dz = q_z - s_j.z   (s_j: source point j, untransformed)
 *   the pair is MUTUAL iff no finite source point j has (d2(j), j) < (d2(i), i) lexicographically -- the library's (distance, lowest index)
 *   argmin rule: of exact duplicates only the lowest index can be mutual; a NaN d2(i) compares below nothing and above nothing: mutual.
 * A pair that is not mutual gets the record {-1, 0.f}; its d2 entry (icp_match's d2_out) stays as the matcher wrote it.  The later stages see
 * the filtered records: icp_iter_stats.n_valid counts what survives them, robust mode ranks the residuals of mutual pairs only.
 * The pose is taken as RIGID: q = R^T (t - T) is the target point in the source's frame only when the 3x3 block is orthonormal.  For the
 * poses ICP produces the test then equals the mutual test in the target's frame up to fp32 rounding.  Parity unpinned (no such stage in the
 * reference); the contract is restated in numpy by tests/reciprocal_restatement.py.
 * The reverse search always runs on a BVH over the source (built on first use, dropped by every call that replaces the source), with either
 * k-NN backend and with projective matching.  Supported: icp_run, icp_iterate, icp_correspond, icp_batch_run, icp_track_depth_frames;
 * every metric, weighting, rejection, multires, selection, robust mode, the convergence stop.  ICP_ERR_INVALID_ARG while on (see
 * icp_last_error): color_icp = 1 (a 6-D forward search against a 3-D reverse one is not a mutual test), the non-linear optimiser,
 * icp_run_multistart, icp_match_seeded.  icp_match and icp_query_matches ignore the option. */
typedef struct icp_reciprocal_options {
    int32_t enabled;   /* 0 (default): no reciprocal test */
} icp_reciprocal_options;
typedef struct icp_reciprocal_stats {   /* one per ICP iteration of the last call */
    int32_t n_matched;   /* pairs judged: queries whose raw match was >= 0 */
    int32_t n_mutual;    /* pairs kept */
} icp_reciprocal_stats;
int icp_reciprocal_options_default(icp_reciprocal_options* opt);
/* Validation: enabled in {0, 1}; else ICP_ERR_INVALID_ARG (reason in icp_last_error). */
int icp_set_reciprocal_options(icp_ctx* ctx, const icp_reciprocal_options* opt);   /* NULL = defaults */
int icp_get_reciprocal_options(const icp_ctx* ctx, icp_reciprocal_options* opt);
/* One record per iteration of the last icp_iterate, icp_run or icp_correspond call on the context (icp_track_depth_frames: the last
 * tracked frame's run; icp_batch_run: each context's own last pair); none when the option was off for that call.  Iterations with no
 * work: {0, 0}.  out[0 .. min(max_out, count)), *count_out = the number of records. */
int icp_get_reciprocal_stats(const icp_ctx* ctx, icp_reciprocal_stats* out, int32_t max_out, int32_t* count_out);

/* -------- ConvergenceMeasure (ConvergenceMeasure.h:30-66): known-correspondence RMSE --------
 * src_xyz[i] (moved by the estimated pose) is compared with ref_xyz[i]; pairs with a non-finite point on either side are skipped.
 * When NO pair is finite, icp_rmse returns ICP_OK and *rmse_out = NaN, as rmseAlignmentError does (:54-65: 0 / 0 under the root);
 * so does the rmse of an iteration record.  icp_benchmark_error skips nothing (calculate_error has no filter): one non-finite point
 * makes it NaN, and a single pair -- its own centroid -- makes it infinite or NaN. */
int icp_set_convergence_reference(icp_ctx* ctx, const float* src_xyz, const float* ref_xyz, int32_t n);
int icp_rmse(icp_ctx* ctx, const float pose[16], float* rmse_out);
/* ConvergenceMeasure::benchmarkError (ConvergenceMeasure.h:104-151): mean |T s_i - r_i| / |T s_i - centroid(T s)|. */
int icp_benchmark_error(icp_ctx* ctx, const float pose[16], float* error_out);

/* -------- utils.h:106-133 on the device (used by the adaptor for transformPoints/Normals) -------- */
int icp_transform_points(icp_ctx* ctx, const float* xyz, int32_t n, const float pose[16], float* out);
int icp_transform_normals(icp_ctx* ctx, const float* normals, int32_t n, const float pose[16], float* out);

/* -------- pre-processing in front of the loop --------
 * PointCloud(float* depthMap, BYTE* colorFrame, depthIntrinsics, depthExtrinsics, width, height, keepOriginalSize, ...)
 * (PointCloud.h:78-165): back-projects a depth image (MINF = no measurement, VirtualSensor.h:119-124) and computes
 * central-difference normals on the device.  Outputs are organised, width*height entries, invalid entries MINF
 * (= keepOriginalSize true, downsampleFactor 1); valid_out (optional) marks the entries the keepOriginalSize = false
 * filter keeps.  rgbx / rgba_out may be NULL.  fix_color_index = 0 reproduces the reference's colour indexing
 * (bytes i..i+3 of the RGBX frame for pixel i, PointCloud.h:156-157), 1 reads pixel i's own 4 bytes. */
int icp_backproject_depth(icp_ctx* ctx, const float* depth, const uint8_t* rgbx, float fx, float fy, float cx, float cy,
                          const float extrinsics[16], int32_t width, int32_t height, float max_distance, int32_t fix_color_index,
                          float* xyz_out, float* normals_out, uint8_t* rgba_out, uint8_t* valid_out);

/* -------- depth frames straight into the resident clouds: PointCloud(depthMap, colorFrame, K, extrinsics, width, height,
 * keepOriginalSize, downsampleFactor, maxDistance) (PointCloud.h:78-165) on the device --------
 * Back-projection and normals as icp_backproject_depth computes them, then the constructor's stride and filter: pixels i = 0, f, 2f, ...
 * (f = downsample_factor), kept when keep_original_size is set or point and normal are both finite, in pixel order.  The kept points go
 * directly into the context's target / source (what icp_set_target / icp_set_source with the same arrays leave, index build included);
 * only the kept-point count comes back to the host (*n_points_out, optional).  depth: width*height fp32 metres, MINF (-inf) = no
 * measurement; rgbx: width*height*4 bytes or NULL (no colours on the cloud).  A frame that keeps no points leaves an empty cloud and
 * returns ICP_ERR_NO_TARGET / ICP_ERR_NO_SOURCE. */
typedef struct icp_depth_camera {
    float fx, fy, cx, cy;            /* depth intrinsics, K(0,0), K(1,1), K(0,2), K(1,2) */
    int32_t width, height;
    float extrinsics[16];            /* depthExtrinsics, column-major (the points are moved by its inverse, the normals are not: PointCloud.h:128-129) */
} icp_depth_camera;
typedef struct icp_depth_options {
    int32_t keep_original_size;      /* keepOriginalSize: keep invalid pixels as MINF entries (organised cloud when downsample_factor == 1) */
    int32_t downsample_factor;       /* >= 1 */
    float   max_distance;            /* maxDistance of the constructor (metres, NOT squared; default 0.1): normals need |gradient| <= max_distance / 2 */
    int32_t fix_color_index;         /* 0: the reference's colour bytes i..i+3 for pixel i (PointCloud.h:156-157); 1: pixel i's own 4 bytes */
} icp_depth_options;
int icp_set_target_depth(icp_ctx* ctx, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_depth_options* opt, int32_t* n_points_out);
int icp_set_source_depth(icp_ctx* ctx, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_depth_options* opt, int32_t* n_points_out);

/* One record per tracked frame k >= 1 of icp_track_depth_frames. */
typedef struct icp_track_frame {
    int32_t n_src;                   /* points the frame kept (source size) */
    int32_t iterations;              /* iterations icp_run ran */
    int32_t status;                  /* ICP_OK, ICP_ERR_NO_SOURCE (frame kept no points: pose carried unchanged) or icp_run's status */
    float   initial_rmse, final_rmse;/* rmseAlignmentError before / after estimatePose (main.cpp:305,311) with gt_frames, else -1 */
    float   pose[16];                /* currentCameraToWorld after frame k, column-major */
} icp_track_frame;
/* The frame-to-reference tracking loop of reconstructRoom (main.cpp:183-341): frame 0 becomes the target (index built once), every later
 * frame k the source of one icp_run with the context's params, starting from pose_inout (currentCameraToWorld, carried from frame to frame).
 * depth_frames: n_frames x width*height fp32; rgbx_frames: n_frames x width*height*4 bytes or NULL (needed for colour ICP / colour
 * weighting).  gt_frames (optional): (n_frames - 1) x 16 floats, the column-major transform of frame k's camera into frame 0's
 * (targetTrajectory * trajectory_k^-1, main.cpp:298-300): the convergence reference of frame k is its source moved by it, built on the
 * device.  Frame k + 1 is uploaded while frame k iterates.  With ICP_MATCH_PROJECTIVE the target options must be (1, 1) and the params'
 * camera must equal cam (ICP_ERR_INVALID_ARG otherwise).  out: n_frames - 1 records.  Returns ICP_OK or the first error in frame order
 * (like icp_batch_run); tracking continues past frames that keep no points.
 * The context keeps what the call left: frame 0 as the target, the last tracked frame as the source and -- with gt_frames -- the last
 * tracked frame's convergence reference, which REPLACES one set earlier with icp_set_convergence_reference (icp_rmse, record_rmse). */
int icp_track_depth_frames(icp_ctx* ctx, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames,
                           const icp_depth_camera* cam, const icp_depth_options* target_opt, const icp_depth_options* source_opt,
                           const float* gt_frames, float pose_inout[16], icp_track_frame* out);

/* -------- the depth mesh reconstructRoom writes after every frame: SimpleMesh(sensor, cameraPose, edgeThreshold) (SimpleMesh.h:36-119)
 * on the device (saveRoomToFile, utils.h:179-193) --------
 * Vertices: all width*height of them, never compacted: MINF (-inf) where the depth is MINF, else the pixel back-projected as
 * icp_backproject_depth does it and moved by cameraPose^-1 (P^-1 E^-1 composed in fp64, both affine, rounded once to fp32).  NaN and
 * +inf depths are not holes: they go through the arithmetic.  Colours: 0 for a MINF pixel, else the RGBX bytes the vertex re-projects
 * to in the colour frame (Kc Ec P composed in fp64, rounded once; floor, the x86-64 (unsigned int) cast, clamped to the frame).
 * Triangles: per 2x2 quad (i0 = i*width + j, i1 = i0 + width, i2 = i0 + 1, i3 = i1 + 1), (i0, i1, i2) then (i1, i3, i2), each kept when
 * its three vertices are finite and every edge is shorter than edge_threshold; in the reference's addFace order.
 * depth: width*height fp32 metres (cam's size limits, and 2 (width - 1)(height - 1) <= INT32_MAX); camera_pose: world -> camera,
 * column-major (reconstructRoom passes currentCameraToWorld^-1).  color_cam NULL = the depth intrinsics, the depth frame size and
 * identity extrinsics (the TUM sensor, VirtualSensor.h:44-51).  rgbx: the colour frame, color width*height*4 bytes; NULL only when
 * colors_out is NULL.  Outputs: vertices_out width*height*3 floats, colors_out (optional) width*height*4 bytes, triangles_out room for
 * 2 (width - 1)(height - 1) * 3 indices, *n_triangles_out the number written.  Uses scratch buffers of the context only (target,
 * source, index, params and convergence reference stay untouched). */
typedef struct icp_color_camera {
    float fx, fy, cx, cy;            /* colour intrinsics, Kc(0,0), Kc(1,1), Kc(0,2), Kc(1,2) */
    int32_t width, height;           /* size of the RGBX colour frame */
    float extrinsics[16];            /* colour extrinsics Ec, column-major */
} icp_color_camera;
int icp_depth_mesh(icp_ctx* ctx, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_color_camera* color_cam,
                   const float camera_pose[16], float edge_threshold, float* vertices_out, uint8_t* colors_out, uint32_t* triangles_out,
                   int32_t* n_triangles_out);

/* -------- frame-to-model tracking (an extension): depth frames fused into a truncated signed distance volume, the volume ray-cast as the
 * target (Newcombe et al., KinectFusion, ISMAR 2011).  DESIGN.md section 6m. --------
 * icp_track_depth_frames aligns every frame to frame 0 and loses the track when the camera turns away from it; here every tracked frame is
 * fused into ONE dense volume per context (device-resident, 8 bytes per voxel) and frame k is aligned to a ray-cast of that volume from the
 * current pose.  With none of these entry points called nothing else in the library changes behaviour.
 * The world is whatever frame the poses live in.  cam->extrinsics must be the identity (the TUM sensor), else ICP_ERR_INVALID_ARG.  `pose` is
 * always camera -> world, column-major (currentCameraToWorld).  Every call but create / options_* needs a volume (ICP_ERR_INVALID_ARG).
 * All fp32 arithmetic is one rounding per operation in the order written (tests/tsdf_restatement.py restates it, compared bit for bit).
 *
 * Integrate: M = pose^-1 (affine inverse in fp64, rounded once).  Voxel (i, j, k): p = (o_x + (float)i s, o_y + (float)j s, o_z + (float)k s);
 *   x_c = (M_00 p_x + (M_01 p_y + M_02 p_z)) + M_03 (y_c, z_c likewise); skipped unless z_c > 0; u = floorf((fx (x_c / z_c) + cx) + 0.5f), v
 *   likewise; skipped unless 0 <= u < width and 0 <= v < height (tested in float); d = depth[v width + u]; skipped unless d is finite, d > 0 and
 *   d <= max_depth; sdf = d - z_c; skipped if sdf < -truncation; f = fminf(1, sdf / truncation); D <- (W D + f) / (W + 1), then
 *   W <- fminf(W + 1, max_weight).  A skipped voxel is neither read nor written.  *n_updated_out (optional): voxels written.
 * Ray-cast: outputs width*height entries in pixel order, in the ray-casting camera's frame, holes MINF, as an organised depth cloud; any
 *   output pointer may be NULL.  Pixel (u, v): a = ((float)u - cx) / fx, b = ((float)v - cy) / fy, dw_r = P_r0 a + (P_r1 b + P_r2 1); at
 *   camera depth z the world point is q_r = P_r3 + z dw_r.  The field at q: g = (q - o) / s per axis, i0 = floor(g), t = g - i0; the sample is
 *   VALID iff 0 <= i0 <= n - 2 on every axis and all eight corner weights are > 0; F = the nested lerp a + t (b - a) along x, then y, then z.
 *   The march: z_k = min_depth + (float)k step for every k with z_k <= max_depth; the ray ends at the first k whose sample is valid with
 *   F_k <= 0 (a NaN never ends a ray); a hit iff k >= 1 and sample k - 1 was valid with F_(k-1) > 0, anything else a hole;
 *   z* = z_(k-1) + step (F_(k-1) / (F_(k-1) - F_k)).  The normal at q(z*): the analytic gradient of that cell's trilinear interpolant (G_x =
 *   the lerp over y then z of the four corner differences along x; G_y over x then z; G_z over x then y; an invalid cell: a hole), n_r =
 *   -(P_0r G_x + (P_1r G_y + P_2r G_z)), normalised as the depth normals are (sq = x x + (y y + z z), / sqrtf(sq)); a non-finite normal: a
 *   hole.  The normal points away from the camera on a surface seen from the front, as the depth normals (-du, -dv, 1) do.
 *   Vertex (a z*, b z*, z*), depth z*, *n_hits_out the number of hits. */
typedef struct icp_tsdf_options {
    int32_t dims[3];                 /* nx, ny, nz >= 2, nx*ny*nz <= INT32_MAX */
    float   origin[3];               /* world position of the CENTRE of voxel (0,0,0) */
    float   voxel_size;              /* > 0 */
    float   truncation;              /* > 0 */
    float   max_weight;              /* >= 1 */
    float   min_depth, max_depth;    /* ray-cast range and integration cut-off, 0 < min < max */
    float   ray_step;                /* 0 = truncation / 2; must be <= truncation; (max_depth - min_depth) / ray_step <= 2^20 */
} icp_tsdf_options;
/* dims 0 (to be set), origin 0, voxel 0.05, truncation 0.25, max weight 64, depth range 0.3 .. 8, ray_step 0. */
int icp_tsdf_options_default(icp_tsdf_options* opt);
/* ICP_OK or ICP_ERR_INVALID_ARG for options icp_tsdf_create would refuse; needs neither a context nor a device. */
int icp_tsdf_options_check(const icp_tsdf_options* opt);
/* create: allocates the context's volume (replacing an earlier one) and clears it (tsdf 0, weight 0); bad options: ICP_ERR_INVALID_ARG with
 * a message.  reset clears it, release frees it (icp_ctx_destroy too). */
int icp_tsdf_create(icp_ctx* ctx, const icp_tsdf_options* opt);
int icp_tsdf_reset(icp_ctx* ctx);
int icp_tsdf_release(icp_ctx* ctx);
/* Two fp32 arrays of nx*ny*nz values, x fastest; either pointer of download may be NULL.  upload: to ray-cast a crafted volume. */
int icp_tsdf_download(icp_ctx* ctx, float* tsdf_out, float* weight_out);
int icp_tsdf_upload(icp_ctx* ctx, const float* tsdf, const float* weight);
int icp_tsdf_integrate(icp_ctx* ctx, const float* depth, const icp_depth_camera* cam, const float pose[16], int32_t* n_updated_out);
int icp_tsdf_raycast(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out, float* normals_out,
                     int32_t* n_hits_out);
/* The same ray-cast written straight into the target as an organised width*height cloud: what icp_set_target leaves for the arrays
 * icp_tsdf_raycast returns, with normals and without colours (index build included); only the hit count comes back (*n_points_out,
 * optional).  No hits: an empty target and ICP_ERR_NO_TARGET.  Source, params and convergence reference stay untouched. */
int icp_set_target_tsdf(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out);
/* Frame-to-model tracking; records as icp_track_depth_frames, one per frame k >= 1.  Frame 0 is integrated at pose_inout.  Frame k:
 * icp_set_target_tsdf at the current pose; frame k becomes the source (source_opt, no colours); one icp_run from the IDENTITY gives dT.  On
 * ICP_OK pose <- pose dT (the fp64 product, each element ((P_r0 D_0c + P_r1 D_1c) + P_r2 D_2c) + P_r3 D_3c, rounded once) and frame k is
 * integrated at the new pose.  A model without hits (ICP_ERR_NO_TARGET), a frame that keeps no points (ICP_ERR_NO_SOURCE) or a failed run
 * (its status): the pose is carried, the frame is not integrated, the status is recorded, tracking goes on; the first error in frame order
 * is returned.  gt_frames: as icp_track_depth_frames (frame k's camera -> the world of pose_inout's first value); the convergence reference
 * of frame k is its source moved by pose_before^-1 gt_k (fp64, rounded once), initial_rmse is taken at the identity, final_rmse at dT.
 * Frame k + 1 goes up while frame k iterates.  With ICP_MATCH_PROJECTIVE the params' camera must equal cam.  Runs with whatever icp_run
 * accepts on such a pair (the non-linear optimiser, robust mode, reciprocal rejection, the convergence stop, the selections);
 * ICP_ERR_INVALID_ARG (see icp_last_error) for what needs target colours (colour ICP, colour weighting, ICP_METRIC_COLORED) and for
 * ICP_METRIC_GICP, whose per-target covariance pass would run every frame. */
int icp_track_depth_model(icp_ctx* ctx, const float* depth_frames, int32_t n_frames, const icp_depth_camera* cam,
                          const icp_depth_options* source_opt, const float* gt_frames, float pose_inout[16], icp_track_frame* out);

/* -------- the model as a mesh (an extension): the zero level set of the context's volume as an indexed triangle mesh with per-vertex
 * normals, extracted on the device; only the mesh crosses to the host.  DESIGN.md section 6n. --------
 * Method: every cell is cut into the six tetrahedra of the Kuhn (Freudenthal) triangulation and each tetrahedron is marched on its own;
 * there are no ambiguous cases and neighbouring cells agree on their shared faces, so the mesh of a closed surface is closed and
 * consistently oriented (about twice the triangles of marching cubes).  All fp32, one rounding per operation in the order written
 * (tests/tsdf_mesh_restatement.py restates it, compared bit for bit).
 * Definitions: a voxel is OBSERVED iff W > 0, W >= min_weight and F is finite (min_weight finite and >= 0; at 0 this is the ray-cast's rule
 *   plus the finiteness test); cell (i, j, k), 0 <= i <= nx - 2 and likewise on the other axes, is VALID iff its eight corners are observed;
 *   a voxel is NEGATIVE iff F < 0.f (zero is not negative).
 * Tetrahedra: tetrahedron pi (a permutation of the axes) of a cell has the corners q0 = (0,0,0), q1 = e_pi0, q2 = e_pi0 + e_pi1,
 *   q3 = (1,1,1); the six come in lexicographic order of pi: xyz, xzy, yxz, yzx, zxy, zyx.  Local edges (0,1), (0,2), (0,3), (1,2), (1,3),
 *   (2,3) have the ranks 0..5.  Case mask m: bit a set iff q_a is negative; m = 0 and m = 15 give nothing.  One corner alone on its side:
 *   one triangle, its three edges in ascending rank.  Two and two (negatives a < b, positives c < d): the quad cycle (a,c), (a,d), (b,d),
 *   (b,c), rotated to start at its smallest rank, as the triangles (e0, e1, e2) and (e0, e2, e3).  Orientation: with every crossing put at
 *   its edge's midpoint, if the normal of the first triangle (right-hand rule; of the second if the first is degenerate) has a negative dot
 *   product with (mean of the positive corners - mean of the negative corners), the order is reversed keeping the first edge: e0 e2 e1, or
 *   e0 e3 e2 e1.  Triangles are therefore counter-clockwise seen from free space (F > 0).
 * Vertices: every tetrahedron edge runs from a voxel v = (i, j, k) to v + d, d in {0,1}^3 \ {0}; it is owned by v under the code
 *   d_x + 2 d_y + 4 d_z (1..7: three axis edges, three face diagonals, the body diagonal; all seven lie in cell v).  An edge carries a
 *   vertex iff exactly one of its ends is negative and at least one valid cell contains it, so every vertex is used by a triangle.  Order:
 *   ascending owner index (k ny + j) nx + i, then ascending code.  Position: t = F_v / (F_v - F_(v+d)), ts = t s; on axes with d_r = 1
 *   p_r = (o_r + (float)i_r s) + ts, on the others p_r = o_r + (float)i_r s.
 * Normals: of the valid cells that contain the edge -- the cells v - off, off_r in {0,1} only on axes with d_r = 0, inside the cell range --
 *   the first in ascending off_x + 2 off_y + 4 off_z; the analytic gradient G of its trilinear interpolant at the local fractions
 *   t_r = d_r ? t : (float)off_r, by the ray-cast's formula and lerp order; n = G / sqrtf(Gx Gx + (Gy Gy + Gz Gz)), in the WORLD frame,
 *   pointing into free space -- the opposite sign convention from icp_tsdf_raycast's camera-frame normal, which points away from the camera,
 *   into the surface.  A non-finite normal is written as (0, 0, 0).
 * Triangles: ascending cell index (x fastest over the (nx-1)(ny-1)(nz-1) cells), valid cells only, then tetrahedron order, then the table's
 *   order; three uint32 vertex indices each.  An exact 0 in the field gives t = 0 or 1: coincident vertices with DISTINCT indices and
 *   zero-area triangles, which are kept; index triples are never degenerate.
 * Calling: *n_vertices_out and *n_triangles_out are always written.  With vertices_out, normals_out and triangles_out all NULL the call only
 *   counts (ICP_OK).  normals_out alone may be NULL.  vertices_out / normals_out: room for max_vertices * 3 floats, triangles_out for
 *   max_triangles * 3 indices; a count above its capacity: ICP_ERR_INVALID_ARG, a message with both counts, nothing written to the arrays.
 *   No volume, a bad min_weight, or a volume of more than INT32_MAX / 12 voxels (a cell gives at most 12 triangles; 512^3 fits):
 *   ICP_ERR_INVALID_ARG.  An empty mesh: ICP_OK with 0 and 0.  Volume, target, source, index, params and convergence reference stay
 *   untouched; scratch comes from the context (1.4375 bytes per voxel, freed with the volume). */
int icp_tsdf_mesh(icp_ctx* ctx, float min_weight, int32_t max_vertices, int32_t max_triangles,
                  float* vertices_out, float* normals_out, uint32_t* triangles_out,
                  int32_t* n_vertices_out, int32_t* n_triangles_out);

/* -------- the coloured model (an extension): a colour array next to the volume, fused, ray-cast, tracked against and meshed with the
 * geometry.  DESIGN.md section 6p. --------
 * The volume gets an optional second array, one float4 (R, G, B, Wc) per voxel, x fastest, indexed as the volume is: R, G, B are running
 * averages of the byte values 0..255 held as floats, Wc is the colour's own weight (its update set is smaller than the geometry's).  fp32 on
 * purpose: the average keeps its bits against tests/tsdf_color_restatement.py and does not stall at Wc = max_weight; a corner is one
 * 16-byte load.  MEMORY: 16 bytes per voxel -- at 512^3 the colour array is 2 GiB next to the 1 GiB of geometry.  icp_tsdf_options keeps its
 * layout: the array is created by its own call.  With none of these entry points called nothing else in the library changes behaviour; every
 * geometry-only call stays legal on a volume with colours and leaves the colour array alone, except: icp_tsdf_reset also clears it,
 * icp_tsdf_release, icp_tsdf_create (replacing a volume) and icp_ctx_destroy free it.  Every call below but icp_tsdf_color_create needs the
 * colour array, else ICP_ERR_INVALID_ARG with a message.  All fp32 arithmetic is one rounding per operation in the order written.
 *
 * color_create: needs a volume; allocates and clears (0, 0, 0, 0); called again it clears.  download / upload: rgb n x 3 and weight n floats,
 *   x fastest, n = nx ny nz; either pointer of download may be NULL.
 * Integrate: geometry, and *n_updated_out, exactly as icp_tsdf_integrate from the same state.  rgbx: the colour frame of the depth frame's
 *   size, registered to it (the TUM sensor), 4 bytes per pixel.  A voxel's colour is updated iff the voxel is updated AND !(sdf > truncation)
 *   -- the band |sdf| <= truncation: free space far in front of a surface would take the colour of what lies behind it.  The pixel is the one
 *   the geometry used, c_r = (float)rgbx[4 (v width + u) + r]; C_r <- (Wc C_r + c_r) / (Wc + 1) per channel, then
 *   Wc <- fminf(Wc + 1, max_weight).  A voxel that is not coloured has its float4 neither read nor written.  *n_colored_out (optional):
 *   voxels coloured.
 * Ray-cast: march, hit, z*, vertex, normal and the first three arrays exactly as icp_tsdf_raycast.  The colour of a hit comes from the cell
 *   of q(z*), the cell of the normal, with its fractions t: all eight corners have Wc > 0: the nested lerp a + t (b - a) along x, then y,
 *   then z, per channel; otherwise the corner nearest the hit, d_r = (t_r >= 0.5f), if its Wc > 0; otherwise no colour.  Byte:
 *   (uint8_t)(int)floorf(fminf(fmaxf(C, 0.f), 255.f) + 0.5f); a coloured pixel is (R, G, B, 255), a hole or an uncoloured hit four zero
 *   bytes.  rgba_out: width*height*4 bytes (may be NULL as the others); *n_colored_out: the coloured hits. */
int icp_tsdf_color_create(icp_ctx* ctx);
int icp_tsdf_color_release(icp_ctx* ctx);
int icp_tsdf_color_download(icp_ctx* ctx, float* rgb_out, float* weight_out);
int icp_tsdf_color_upload(icp_ctx* ctx, const float* rgb, const float* weight);
int icp_tsdf_integrate_color(icp_ctx* ctx, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16],
                             int32_t* n_updated_out, int32_t* n_colored_out);
int icp_tsdf_raycast_color(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out,
                           float* normals_out, uint8_t* rgba_out, int32_t* n_hits_out, int32_t* n_colored_out);
/* icp_set_target_tsdf WITH colours: what icp_set_target leaves for the arrays icp_tsdf_raycast_color returns once its uncoloured hits are
 * turned into holes (every consumer of a coloured target needs the colour; a caller who does not has icp_set_target_tsdf).  *n_points_out:
 * the coloured hits; none: an empty target and ICP_ERR_NO_TARGET. */
int icp_set_target_tsdf_color(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out);
/* icp_track_depth_model with four changes: frames are staged with their colour frame (rgbx_frames: n_frames x width*height*4 bytes), the
 * target comes from icp_set_target_tsdf_color, the source is built with colours, integration is icp_tsdf_integrate_color.  Accepts colour
 * ICP (6-D k-NN), ICP_WEIGHT_COLORS and ICP_METRIC_COLORED, whose per-target gradient pass then runs every frame.  ICP_ERR_INVALID_ARG for
 * GICP, null rgbx_frames, a volume without colours, and source_opt->fix_color_index == 0: the model holds each pixel's own bytes, the
 * reference's shifted bytes on the source side would compare unlike things. */
int icp_track_depth_model_color(icp_ctx* ctx, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                                const icp_depth_options* source_opt, const float* gt_frames, float pose_inout[16], icp_track_frame* out);
/* icp_tsdf_mesh with a colour per vertex: counts, vertices, normals and triangles are icp_tsdf_mesh's.  colors_out: max_vertices * 4 bytes,
 * may be NULL.  The vertex on the edge from v to v + d at its t: both ends have Wc > 0: C_v + t (C_(v+d) - C_v) per channel; one end has:
 * that end's colour; neither: four zero bytes.  Bytes by the ray-cast's rule, alpha 255. */
int icp_tsdf_mesh_color(icp_ctx* ctx, float min_weight, int32_t max_vertices, int32_t max_triangles,
                        float* vertices_out, float* normals_out, uint8_t* colors_out, uint32_t* triangles_out,
                        int32_t* n_vertices_out, int32_t* n_triangles_out);

/* -------- direct SDF tracking (an extension): a depth frame aligned to the volume itself, without ray-cast, target cloud, index or search
 * (Bylow, Sturm, Kerl, Kahl, Cremers, RSS 2013; Canelhas et al., IROS 2013).  DESIGN.md section 6q. --------
 * The volume stores a signed distance and its gradient is the surface normal: a depth pixel moved into the world reads its residual and its
 * normal from the eight voxels around it.  Each Gauss-Newton step is the library's point-to-plane step (row [q x g, g], right-hand side -r).
 * Needs a volume and identity depth extrinsics as the calls above do; the alignment of these geometric calls never reads the colour array
 * (the calls of the next block do).  Target, source, index, params
 * and convergence reference stay untouched.  All fp32 arithmetic is one rounding per operation in the order written; everything after the
 * conversion to fp64 is fp64, one rounding per operation (tests/sdf_restatement.py restates it).
 *
 * Sampled pixels: (u, v) with u % stride == 0 and v % stride == 0.  A sampled pixel is USABLE iff its depth d is finite, d > 0 and
 *   d <= max_depth (the integrate rule's tests); n_depth counts them.
 * Field sample: a = ((float)u - cx) / fx, b = ((float)v - cy) / fy, x = a d, y = b d; q_r = (P_r0 x + (P_r1 y + P_r2 d)) + P_r3 with P the
 *   camera -> world pose.  The cell of q, its validity, F and the analytic gradient (G_x, G_y, G_z) are the ray-cast's (above).  The pixel is
 *   VALID iff it is usable, its cell is valid and fabsf(F) < 1: a NaN drops out, and a sample clamped at the free-space value carries no
 *   gradient.  n_valid counts them.
 * Terms, in fp64: r = (double)F (double)truncation [m]; g = (double)G ((double)truncation / (double)voxel_size);
 *   J = (q_y g_z - q_z g_y, q_z g_x - q_x g_z, q_x g_y - q_y g_x, g_x, g_y, g_z) with q converted; w = 1, or with huber > 0:
 *   w = |r| <= huber ? 1 : huber / |r|.
 * Sums: 28 doubles -- (w J_i) J_j, the upper triangle of sum w J J^T, entry (i, j >= i) at i 6 - i (i - 1) / 2 + (j - i); the six
 *   -((w J_i) r) at 21 + i; (w r) r at 27.  They are folded in a fixed order without floating-point atomics: bitwise reproducible run to
 *   run; against another summation order each differs by at most n_valid 2^-52 sum |term|.
 * Step: fails when n_valid < min_valid.  Else the 27 sums are solved as the point-to-plane metric solves its own (the LDL^T path; where
 *   its rank guard refuses, the truncated eigen-solve), x = (alpha, beta, gamma, t), and pose <- dT pose with dT = [Rx Ry Rz | t] composed
 *   in fp32 as there.  A non-finite x or pose fails the step.
 * Stop: after a successful step, when every |angle| <= stop_rotation and every |t_i| <= stop_translation (fp64 x against the fp32 bounds);
 *   either bound at 0 turns the stop off.  A frame ends at the stop, at a failed step, or after n_iterations; what is still enqueued of it
 *   returns at once, and nothing crosses to the host between iterations.
 * A frame FAILS with no usable pixel (ICP_ERR_NO_SOURCE) or a failed step (ICP_ERR_NO_CORRESPONDENCES): it carries the pose it started with. */
typedef struct icp_sdf_options {
    int32_t stride;                  /* >= 1, default 1 */
    int32_t n_iterations;            /* 1 .. 1000, default 20 */
    int32_t min_valid;               /* >= 6, default 64 */
    float   huber;                   /* metres, >= 0, default 0 = off */
    float   stop_rotation, stop_translation;   /* >= 0, default 1e-5 each */
} icp_sdf_options;
typedef struct icp_sdf_iter {
    int32_t n_valid, status;         /* of the sums taken at the pose BEFORE the step; the step's status */
    double  cost;                    /* sum w r r there */
    float   pose[16];                /* the pose AFTER the step (a failed step: the pose it was taken at) */
} icp_sdf_iter;
typedef struct icp_sdf_frame {
    int32_t n_depth, n_valid_first, n_valid_last, iterations, status;   /* iterations: the steps tried, a failed one included */
    double  cost_first, cost_last;   /* sum w r r at the first and at the last pose the sums were taken at */
    float   pose[16];
} icp_sdf_frame;
int icp_sdf_options_default(icp_sdf_options* opt);
/* ICP_OK or ICP_ERR_INVALID_ARG; needs neither a context nor a device. */
int icp_sdf_options_check(const icp_sdf_options* opt);
/* The field and its gradient at n >= 0 world points (n x 3): f_out n floats, grad_out n x 3 floats (G, per voxel), valid_out n bytes (the
 * cell is valid); any output may be NULL.  An invalid point reads F = 0, G = 0; a NaN is stored as the canonical quiet NaN 0x7FC00000. */
int icp_tsdf_sample(icp_ctx* ctx, const float* points, int32_t n, float* f_out, float* grad_out, uint8_t* valid_out);
/* The sums of ONE step at `pose`: sums_out 28 doubles, counts_out {n_depth, n_valid}; of opt only stride and huber matter. */
int icp_tsdf_sdf_system(icp_ctx* ctx, const float* depth, const icp_depth_camera* cam, const float pose[16], const icp_sdf_options* opt,
                        double* sums_out, int32_t* counts_out);
/* Aligns one frame to the volume from pose_inout.  rec_out (optional): the frame's record; trace_out: NULL, or n_iterations records, those
 * past the last step tried zeroed.  Returns the frame's status; a failed frame leaves pose_inout as it was. */
int icp_tsdf_align_depth(icp_ctx* ctx, const float* depth, const icp_depth_camera* cam, const icp_sdf_options* opt, float pose_inout[16],
                         icp_sdf_frame* rec_out, icp_sdf_iter* trace_out);
/* Tracking: frame 0 is integrated at pose_inout; frame k >= 1 is aligned from the current pose and, on ICP_OK, integrated at the pose found
 * (out[k - 1] its record).  A failed frame carries the pose, is not integrated, records its status, and tracking goes on; the first error
 * in frame order is returned.  rgbx_frames: NULL, or the colour frames (n_frames x width*height*4 bytes) for a volume that has the colour
 * array: integration is then icp_tsdf_integrate_color.  Frame k + 1 goes up while frame k iterates; the host reads one frame record per
 * frame.  ICP_ERR_INVALID_ARG (see icp_last_error) for no volume, non-identity depth extrinsics, bad options, or rgbx_frames without a
 * colour array. */
int icp_track_depth_sdf(icp_ctx* ctx, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                        const icp_sdf_options* opt, float pose_inout[16], icp_sdf_frame* out);

/* -------- the hashed TSDF volume (an extension): the volume above without a fixed extent, in blocks of 8 x 8 x 8 voxels that a hash table
 * addresses by block coordinates (Niessner, Zollhoefer, Izadi, Stamminger, "Real-time 3D Reconstruction at Scale using Voxel Hashing",
 * SIGGRAPH Asia 2013).  DESIGN.md section 6x. --------
 * The dense volume is a box fixed before the first frame, 8 bytes per voxel whatever the voxel holds; a track that leaves the box is lost
 * without an error.  The hashed volume allocates blocks on the device from each depth frame, around the surface alone, and direct SDF
 * tracking runs on it as it is.  A context holds ONE volume, dense or hashed; icp_tsdf_create_hashed replaces either.
 * tests/htsdf_restatement.py restates what follows, compared bit for bit.
 *
 * Storage: a block is 8 x 8 x 8 voxels, one (tsdf, weight) pair each, x fastest (4 KiB).  Voxel g (signed global coordinates) belongs to
 *   block b = g >> 3 (arithmetic shift) at local index g & 7; its world position is o + (float)g s per axis, the dense formula with a signed
 *   index.  Options are icp_tsdf_options with dims ignored.  Block coordinates are storable in -2^20 <= b < 2^20.  A table of keys maps a
 *   block to its index in a POOL of blocks (what costs memory: block_capacity blocks of 4 KiB, plus 12 bytes per table slot and 8 per
 *   block; the table has at least 2 slots per pool block).  Where a block sits in the pool may depend on a race; what it holds does not.
 *   A voxel of a block that is not allocated reads as (0, 0): unobserved.
 * Touch (allocation, in front of every integrate, decided from the depth frame and the pose alone): for each pixel (u, v) with finite d,
 *   0 < d <= max_depth: a = ((float)u - cx) / fx, b = ((float)v - cy) / fy; for m = 0 .. M, M = ceil(2 truncation / s) (in double):
 *   z_m = fminf((d - truncation) + (float)m s, d + truncation), skipped unless z_m > 0; q_r = (P_r0 (a z_m) + (P_r1 (b z_m) + P_r2 z_m)) + P_r3;
 *   the cell is f = floorf((q - o) / s) per axis.  A sample with -2^23 <= f <= 2^23 - 2 on every axis (tested in float; the blocks of its
 *   eight corners are then storable) allocates the blocks (f + {0, 1}) >> 3 of those corners; any other sample allocates nothing and is
 *   counted in n_out_of_range.  The SET of blocks is exact and does not depend on the order of anything.
 * Room: a block that finds no table slot or no pool block is counted (n_unplaced) and gets no storage; the host reads the touch's
 *   counters, and if anything was unplaced it doubles table and pool (live blocks rehashed, no trace of the failed claims), and runs the
 *   touch again -- it is idempotent -- until nothing is unplaced; only then is the integrate launched.  Growth beyond 2^22 blocks (16 GiB) is
 *   refused with ICP_ERR_INVALID_ARG and a message, the volume as it was before the call.
 * Integrate: the dense rule on every voxel of every allocated block, with (float)g for (float)i; *n_updated_out counts the voxels written.
 * Field: the dense sample with the cell f tested against -2^23 <= f <= 2^23 - 2 in place of the box; VALID iff the blocks of all eight
 *   corners exist and all eight weights are > 0.  F, G, the residual, the Jacobian, the sums and the solve are those of direct SDF tracking.
 * icp_tsdf_reset and icp_tsdf_release work on either storage (reset keeps the capacity); icp_tsdf_integrate, icp_tsdf_sample,
 *   icp_tsdf_sdf_system, icp_tsdf_align_depth and icp_track_depth_sdf (without colour frames) work on whichever volume the context holds,
 *   with the same options, records and statuses.  On a hashed volume an integrate waits for the host twice (the touch's counters, the
 *   update count) and a tracked frame twice (its record, the touch's counters); the dense loop waits once per frame.
 * Refused on a hashed volume (ICP_ERR_INVALID_ARG, a message that names the hashed volume, no side effect): icp_tsdf_download,
 *   icp_tsdf_upload, icp_tsdf_raycast*, icp_set_target_tsdf*, icp_track_depth_model* (the hashed volume's own calls are icp_tsdf_raycast_hashed,
 *   icp_set_target_tsdf_hashed and icp_track_depth_model_hashed, below), icp_tsdf_mesh (the hashed volume's own mesh call is icp_tsdf_mesh_hashed,
 *   below), icp_tsdf_color_create and every *_color call -- on a hashed volume WITHOUT colours; what a coloured one (icp_tsdf_create_color_hashed,
 *   further below) accepts is listed there.  A finished model goes into a dense volume block by block (icp_get_tsdf_hashed, then icp_tsdf_upload). */
typedef struct icp_tsdf_hashed_info {
    int32_t n_blocks;                /* allocated blocks */
    int32_t capacity;                /* blocks the pool holds before it grows */
    int32_t n_grown;                 /* growths since create */
    int32_t n_unplaced;              /* nonzero: claims of the last touch / allocate found no storage (not a tally; 0 after every successful call) */
    int64_t n_out_of_range;          /* samples skipped because their cell is not storable, since create / reset / upload */
} icp_tsdf_hashed_info;
/* create: opt as for icp_tsdf_create (dims ignored); block_capacity in 1 .. 2^22, rounded up to a power of two. */
int icp_tsdf_create_hashed(icp_ctx* ctx, const icp_tsdf_options* opt, int32_t block_capacity);
/* Grows table and pool ahead of time so that `block_capacity` blocks fit without a growth (never shrinks). */
int icp_tsdf_reserve_blocks(icp_ctx* ctx, int32_t block_capacity);
/* Allocates the n blocks coords[3 i .. 3 i + 2] (storable, else ICP_ERR_INVALID_ARG; one named twice or allocated already: no effect)
 * under the room rule. */
int icp_tsdf_allocate_blocks(icp_ctx* ctx, int32_t n, const int32_t* coords);
/* The blocks SORTED BY KEY (z, then y, then x of the block coordinate): coords_out n_blocks x 3, tsdf_out and weight_out n_blocks x 8 x 8 x 8
 * (z, y, x; x fastest).  Every pointer may be NULL; with an array asked for, max_blocks below n_blocks is ICP_ERR_INVALID_ARG. */
int icp_get_tsdf_hashed(icp_ctx* ctx, icp_tsdf_hashed_info* info_out, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out);
/* REPLACES the state with n blocks in icp_get_tsdf_hashed's layout (storable, none twice, else ICP_ERR_INVALID_ARG); the counters restart. */
int icp_tsdf_upload_hashed(icp_ctx* ctx, int32_t n, const int32_t* coords, const float* tsdf, const float* weight);

/* -------- streaming the hashed volume (an extension): the blocks beyond a radius of the camera leave the device for the host and come back
 * when the camera returns (Niessner et al., section 5), so device memory and the integrate's cost are bounded by what is in reach while
 * the model stays complete on the host.  DESIGN.md section 6za.  tests/htsdf_evict_restatement.py restates what follows. --------
 * Rule of evict(centre, radius): it applies to every pool block 0 .. n_blocks - 1.  With b the block's coordinates (from its key), o and s
 *   the volume's origin and voxel size, in fp32, operation for operation, without contraction:
 *     p_a = o_a + ((float)(8 b_a) + 3.5f) * s      (the centre of the block's 512 voxel positions)
 *     d_a = p_a - centre_a,   d2 = (d_x d_x + d_y d_y) + d_z d_z
 *   the block is KEPT iff d2 <= r2, with r2 = radius * radius computed once on the host in fp32; an infinite r2 keeps everything.  This
 *   is icp_voxel_map_prune's rule with a block's centre in place of a cell's.  centre must be finite, radius finite and >= 0.
 * After icp_tsdf_evict_blocks the volume holds exactly the kept blocks, bit for bit; n_blocks is their number; the pool entries
 *   n_blocks .. capacity - 1 read (0, 0) and carry no key, as after create, so a later touch hands out fresh blocks; the table holds the
 *   kept keys and nothing else (it is cleared and rebuilt: linear probing cannot delete a key).  capacity, n_grown and n_out_of_range do
 *   not change.  The state equals, through every public call, that of a fresh volume that icp_tsdf_upload_hashed filled with the kept
 *   blocks.  If no block is evicted nothing at all is modified.  Where a kept block sits in the pool afterwards may depend on a race (the
 *   kept blocks at or above n_blocks move into the holes below it); what the volume holds does not.
 * hold != 0: the evicted blocks and their keys are first copied into a device-side OUTBOX that the context owns; icp_tsdf_evicted_blocks
 *   returns it in icp_get_tsdf_hashed's layout, sorted by key (max_blocks below n_held: ICP_ERR_INVALID_ARG, the message names both).  The
 *   outbox lives until the next evict, reset, release, create or upload.  hold == 0: the evicted blocks are forgotten.
 * icp_tsdf_insert_blocks ADDS n blocks in icp_get_tsdf_hashed's layout to the existing state (icp_tsdf_upload_hashed REPLACES it).  It
 *   refuses with ICP_ERR_INVALID_ARG and a reason, before anything is modified: a coordinate that is not storable, one that occurs twice,
 *   and any key that is resident already (counted on the device; the count is in the message and in n_present).  Otherwise the blocks
 *   are allocated under the room rule (the pool grows where it must) and their voxels placed.
 * Both calls refuse a context without a volume and one with a dense volume, with a message that names the call.
 * Host waits: an evict waits once when nothing leaves (the mark's counters) and twice otherwise; an insert once for the resident count, once
 *   per room-rule launch and once per slab of 4096 blocks. */
typedef struct icp_tsdf_stream_info {
    int32_t n_evicted;               /* evict: blocks that left */
    int32_t n_blocks;                /* allocated blocks after the call */
    int32_t n_moved;                 /* evict: kept blocks that changed their place in the pool */
    int32_t capacity;                /* blocks the pool holds before it grows */
    int32_t n_held;                  /* evict: blocks in the outbox after the call (n_evicted with hold != 0, else 0) */
    int32_t n_inserted;              /* insert: blocks added */
    int32_t n_present;               /* insert: keys that were resident already (nonzero: the call was refused) */
    int32_t n_grown;                 /* growths since create */
} icp_tsdf_stream_info;
#ifdef __cplusplus
static_assert(sizeof(icp_tsdf_stream_info) == 32, "icp_tsdf_stream_info");
#endif
int icp_tsdf_evict_blocks(icp_ctx* ctx, const float centre[3], float radius, int32_t hold, icp_tsdf_stream_info* info_out);
int icp_tsdf_evicted_blocks(icp_ctx* ctx, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out);
int icp_tsdf_insert_blocks(icp_ctx* ctx, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, icp_tsdf_stream_info* info_out);

/* -------- the coloured hashed volume (an extension): the hashed volume with the colour array of the coloured model (icp_tsdf_color_create)
 * in its blocks, so that colour fusion and the photometric term of direct SDF tracking work without an extent.  DESIGN.md section 6zb.
 * tests/htsdf_color_restatement.py restates what follows, compared bit for bit. --------
 * Storage: icp_tsdf_create_color_hashed is icp_tsdf_create_hashed plus a SECOND POOL: one fp32 (R, G, B, Wc) per voxel, 512 per block
 *   (8 KiB), x fastest, indexed by the pool index of the geometry block, in a buffer of its own (12 KiB per block in all; the geometry-only
 *   kernels read and write what they did).  It is cleared to (0, 0, 0, 0) when allocated, grows with the pool (the live prefix of both
 *   pools is copied), is cleared by icp_tsdf_reset and freed by icp_tsdf_release, create and destroy.  icp_tsdf_hashed_has_color tells
 *   which kind the context holds (ICP_ERR_INVALID_ARG without a hashed volume).  icp_tsdf_hashed_info is unchanged.
 *   A hashed volume WITHOUT colours behaves exactly as before: it refuses every *_color call with the message it always gave.
 * Fusion: icp_tsdf_integrate_color on a coloured hashed volume is the touch under the room rule, then over every allocated block the
 *   hashed integrate's geometry, operation for operation, and the dense coloured rule: a voxel is painted iff it is updated AND
 *   !(sdf > truncation), from the pixel the geometry used, C <- (Wc C + c) / (Wc + 1) per channel, Wc <- fminf(Wc + 1, max_weight); a
 *   voxel that is not painted has its colour neither read nor written.  Both counts as on the dense volume.  icp_tsdf_integrate stays
 *   legal and leaves the colours alone; icp_track_depth_sdf given colour frames fuses them.
 * Save and restore: icp_get_tsdf_color_hashed is icp_get_tsdf_hashed with rgb_out (n_blocks x 512 x 3) and cweight_out (n_blocks x 512) in
 *   the same order and voxel layout, any output NULL; icp_tsdf_upload_color_hashed REPLACES the state with blocks and their colours.
 *   icp_tsdf_upload_hashed on a coloured volume replaces the state and leaves every block uncoloured.
 * Intensity field and photometric tracking: icp_tsdf_sample_color, icp_tsdf_sdf_system_color, icp_tsdf_align_depth_color and
 *   icp_track_depth_sdf_color work on a coloured hashed volume with the same signatures, options, records and statuses.  A colour sample
 *   is VALID iff the cell is storable (-2^23 <= f <= 2^23 - 2, tested in float), the blocks of all eight corners exist and every corner
 *   has Wc > 0; the geometry's weights play no part.  The joint step is the hashed geometric row with the dense photometric row added
 *   into it in that contract's term order; the colour corners are those of the cell the distance was read in.
 * Streaming: icp_tsdf_evict_blocks compacts both pools by the same plan (a mover's colours go into the hole its geometry goes into), with
 *   hold != 0 the outbox receives both, and both tails are cleared: afterwards the volume equals, through every public call and bit for
 *   bit, a fresh coloured volume that icp_tsdf_upload_color_hashed filled with the kept blocks.  icp_tsdf_evicted_blocks_color returns the
 *   outbox with its colours, icp_tsdf_insert_blocks_color adds blocks with theirs (the same refusals as icp_tsdf_insert_blocks).
 *   icp_tsdf_evicted_blocks returns the outbox's geometry; icp_tsdf_insert_blocks leaves the new blocks uncoloured.  The reach of a view
 *   needs no change: the colour is read and written only in cells and voxels the geometry touches.
 * Still refused on a coloured hashed volume (ICP_ERR_INVALID_ARG, a message that names the call, no side effect): icp_tsdf_color_create,
 *   icp_tsdf_color_release, icp_tsdf_color_download and icp_tsdf_color_upload (they address the dense array; the message points at the
 *   calls below), icp_tsdf_raycast_color, icp_set_target_tsdf_color, icp_track_depth_model_color and icp_tsdf_mesh_color (the dense-named
 *   calls; their forms on the blocks are icp_tsdf_raycast_color_hashed, icp_set_target_tsdf_color_hashed,
 *   icp_track_depth_model_color_hashed and icp_tsdf_mesh_color_hashed, further down), with every dense-box call listed above.
 * Legal and geometry-only on a coloured hashed volume: icp_tsdf_mesh_hashed, icp_tsdf_raycast_hashed, icp_set_target_tsdf_hashed and
 *   icp_track_depth_model_hashed; the model loop's own fusion there leaves the colours alone.
 * The new calls refuse a context without a volume, one with a dense volume and one with a hashed volume without colours. */
int icp_tsdf_create_color_hashed(icp_ctx* ctx, const icp_tsdf_options* opt, int32_t block_capacity);
int icp_tsdf_hashed_has_color(icp_ctx* ctx, int32_t* has_out);
int icp_get_tsdf_color_hashed(icp_ctx* ctx, icp_tsdf_hashed_info* info_out, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out,
                              float* rgb_out, float* cweight_out);
int icp_tsdf_upload_color_hashed(icp_ctx* ctx, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb,
                                 const float* cweight);
int icp_tsdf_evicted_blocks_color(icp_ctx* ctx, int32_t max_blocks, int32_t* coords_out, float* tsdf_out, float* weight_out, float* rgb_out,
                                  float* cweight_out);
int icp_tsdf_insert_blocks_color(icp_ctx* ctx, int32_t n, const int32_t* coords, const float* tsdf, const float* weight, const float* rgb,
                                 const float* cweight, icp_tsdf_stream_info* info_out);

/* -------- the hashed model as a mesh (an extension): icp_tsdf_mesh on the block pool -- the zero level set of the context's HASHED volume
 * as an indexed triangle mesh with per-vertex normals; only the mesh crosses to the host and scratch scales with the blocks in use, not with
 * an extent.  DESIGN.md section 6y.  tests/htsdf_mesh_restatement.py restates what follows, compared bit for bit. --------
 * The geometry is icp_tsdf_mesh's (tetrahedra, case table, orientation: see there), read through the hashed volume's addressing:
 * Definitions: a voxel is a signed global coordinate g; it lies in block b = g >> 3 at local index (g_z & 7) 64 + (g_y & 7) 8 + (g_x & 7).  A
 *   voxel of a block that does not exist reads (0, 0): unobserved, not negative.  A voxel is OBSERVED iff W > 0, W >= min_weight and F is
 *   finite, NEGATIVE iff F < 0.f.  Cell g (lowest corner g, corners g + {0,1}^3) is VALID iff its eight corners are observed; it belongs to
 *   the block of g, its corners may lie in up to 8 blocks.  There is no cell range: a cell exists wherever its lowest corner's block does.
 * Vertices: the edge v -> v + d, d in {0,1}^3 \ {0}, is owned by v under the code d_x + 2 d_y + 4 d_z; v + d may lie in a neighbouring
 *   block.  It carries a vertex iff exactly one end is negative and a valid cell v - off, (off & d) == 0, contains it (those cells may lie
 *   in the lower neighbouring blocks).  Position: t = F_v / (F_v - F_(v+d)), ts = t s; per axis base_r = o_r + (float)g_r s with g the SIGNED
 *   GLOBAL coordinate of v; p_r = base_r + ts on axes with d_r = 1, p_r = base_r on the others.
 * Normals: icp_tsdf_mesh's formula and lerp order on the first valid holding cell in ascending off, whose eight corners may span blocks;
 *   normalised, (0, 0, 0) where not finite.
 * Order: where a block sits in the pool depends on a race, the output does not.  Blocks come in ascending key order -- z, then y, then x of
 *   the block coordinate, icp_get_tsdf_hashed's order; a block's position in it is its RANK.  Inside a block voxels come in local linear
 *   order, x fastest.  Vertices: ascending (rank of the owner's block, local index, code).  Triangles: ascending (rank of the cell's block,
 *   local index of the cell's lowest corner, tetrahedron, table order).  An exact 0 gives coincident vertices with DISTINCT indices, kept.
 *   Two volumes with the same blocks give identical arrays, however the blocks were allocated and however often the volume grew.
 *   As a SET of triangles with their corner positions and normals the result is icp_tsdf_mesh's on the dense volume over the bounding box
 *   of the blocks (voxels no block covers (0, 0)), bit for bit wherever that volume's shifted origin o + (float)lo s is exact.
 * Calling: icp_tsdf_mesh's -- the two count pointers are required and always written; all three arrays NULL counts; vertices_out and
 *   triangles_out go together, normals_out alone may be NULL; a count above its capacity: ICP_ERR_INVALID_ARG, both counts returned, a
 *   message with the four numbers, nothing written to the arrays; min_weight finite and >= 0.  No volume: ICP_ERR_INVALID_ARG ("no volume").
 *   A dense volume: ICP_ERR_INVALID_ARG (the message names the dense volume), nothing touched -- icp_tsdf_mesh is the call for it, and it
 *   keeps refusing a hashed one.  No block, or no sign change: ICP_OK with 0 and 0.  n_blocks * 512 > INT32_MAX / 12: ICP_ERR_INVALID_ARG.
 *   The volume is never modified (table, pool, counters, options).  The host reads the blocks' keys (8 bytes per block), sorts them and
 *   uploads the order on every call: one host wait more than icp_tsdf_mesh; nothing is cached between calls.  Scratch comes from the
 *   context (about 850 bytes per block next to the block's 4 KiB, freed with the volume). */
int icp_tsdf_mesh_hashed(icp_ctx* ctx, float min_weight, int32_t max_vertices, int32_t max_triangles,
                         float* vertices_out, float* normals_out, uint32_t* triangles_out,
                         int32_t* n_vertices_out, int32_t* n_triangles_out);

/* -------- the hashed model seen from a pose, and tracked frame-to-model (an extension): icp_tsdf_raycast, icp_set_target_tsdf and
 * icp_track_depth_model on the HASHED volume.  DESIGN.md section 6z.  tests/htsdf_raycast_restatement.py restates what follows, compared bit
 * for bit. --------
 * The ray-cast is icp_tsdf_raycast's, read through the hashed volume's addressing; nothing else changes.
 * March: z_k = min_depth + (float)k ray_step while z_k <= max_depth, all from the volume's icp_tsdf_options (ray_step 0 is truncation / 2).
 *   Every sample of the march is evaluated, in order; none is skipped.
 * Per sample: the direction, the position q = P[12..14] + z d, the nested lerp (x, then y, then z), the end rule, zh and the analytic
 *   gradient normal are icp_tsdf_raycast's, operation for operation in the same order.  The end rule: the ray ends at the first VALID
 *   sample with F <= 0; the crossing is accepted only when the sample before it was valid with F > 0; a NaN never ends a ray; an
 *   invalid sample clears prev_valid.
 * Cell: g = (q - o) / s per axis, f = floor(g), fractions g - f; the corner (dx, dy, dz) is the voxel at SIGNED GLOBAL coordinate f + d,
 *   in block (f + d) >> 3 at local index ((f + d) & 7).
 * Validity: a sample is VALID iff -2^23 <= f <= 2^23 - 2 on every axis (tested in float, before any cast: a NaN or a coordinate out of
 *   range is invalid) and all eight corners have W > 0.  A voxel of a block that does not exist reads (0, 0), so a cell that touches a
 *   missing block is invalid.  There is no box and no cell range beyond storability.
 * Outputs: icp_tsdf_raycast's -- depth (h, w), vertices and normals (w h, 3) in the camera's frame, -inf in all of them where the ray
 *   misses, the number of hits; as a target (icp_set_target_tsdf_hashed) the SoA planes with +inf padding to the next multiple of 64.
 * Determinism: the output is per pixel and reads the volume only through block coordinates: where a block sits in the pool does not
 *   matter, and two volumes with the same blocks give identical arrays.
 * Equivalence: on a volume whose blocks all have non-negative coordinates the result equals icp_tsdf_raycast's on the dense volume with the
 *   same origin and voxel_size that holds the blocks from voxel (0, 0, 0) on and covers every one of them (voxels no block covers (0, 0)),
 *   bit for bit, array for array.
 * The volume is never modified (table, pool, counters, options).
 * icp_tsdf_raycast_hashed: icp_tsdf_raycast's calling rules -- any output may be NULL; one host wait.
 * icp_set_target_tsdf_hashed: icp_set_target_tsdf's -- the ray-cast straight into the target's planes, the target's index built, the hit
 *   count alone downloaded; no hit: ICP_ERR_NO_TARGET and an empty target.
 * icp_track_depth_model_hashed: icp_track_depth_model's loop, arguments, frame records, statuses, carried pose on a failed frame, upload
 *   overlap and gt RMSE, with the target from the hashed ray-cast and the integrate icp_tsdf_integrate's on a hashed volume (the touch with
 *   its growth and room rule; growth past 2^22 blocks ends the call with ICP_ERR_INVALID_ARG).  It keeps that loop's refusals: colour ICP,
 *   colour weighting and the colored metric (the loop reads no colours, also on a coloured hashed volume, whose colours its own fusion leaves alone: the coloured loop of the blocks is icp_track_depth_model_color_hashed, below), GICP, and a projective camera
 *   in the params that differs from the depth camera.  Host waits per tracked frame: icp_track_depth_model's (the hit count, the run's)
 *   and the touch's counters, plus one per growth of the pool.
 * All three: no volume, or a dense volume: ICP_ERR_INVALID_ARG with a message that names the call, nothing touched -- the dense volume's
 *   calls are icp_tsdf_raycast, icp_set_target_tsdf and icp_track_depth_model, which keep refusing a hashed one. */
int icp_tsdf_raycast_hashed(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out,
                            float* normals_out, int32_t* n_hits_out);
int icp_set_target_tsdf_hashed(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out);
int icp_track_depth_model_hashed(icp_ctx* ctx, const float* depth_frames, int32_t n_frames, const icp_depth_camera* cam,
                                 const icp_depth_options* source_opt, const float* gt_frames, float pose_inout[16], icp_track_frame* out);

/* -------- the coloured hashed model seen from a pose, as a coloured target, tracked frame-to-model and meshed (an extension):
 * icp_tsdf_raycast_color, icp_set_target_tsdf_color, icp_track_depth_model_color and icp_tsdf_mesh_color on the blocks of a COLOURED HASHED
 * volume (icp_tsdf_create_color_hashed).  DESIGN.md section 6zc.  tests/htsdf_color_view_restatement.py restates what follows, compared bit
 * for bit. --------
 * Every rule is an existing contract read through the other addressing; there is no new arithmetic.
 * Coloured ray-cast (icp_tsdf_raycast_color_hashed): the march, validity, end rule, zh, the normal, the first three arrays and the hit
 *   count are icp_tsdf_raycast_hashed's, operation for operation.  The colour of a hit is icp_tsdf_raycast_color's rule on the cell of
 *   q(z*), the normal's cell, with its fractions (t_x, t_y, t_z): all eight corners have Wc > 0 -- the nested lerp x, then y, then z, per
 *   channel; otherwise the corner nearest the hit (t_r >= 0.5f picks the upper one) if its Wc > 0; otherwise none.  Bytes by
 *   floor(clamp(c, 0, 255) + 0.5), packed R | G << 8 | B << 16 | 255 << 24.  Corner (dx, dy, dz) is the colour-pool entry of the voxel at
 *   signed global coordinate f + d, read through the block index that the geometry lookup of that same cell found: no second table probe,
 *   and colour corners are loaded for that one cell per ray only.  A hole or an uncoloured hit is four zero bytes; *n_colored_out counts
 *   the coloured hits.  Any output may be NULL; one host wait.
 *   Equivalence: on blocks at non-negative coordinates the result equals icp_tsdf_raycast_color's bit for bit, all four arrays and both
 *   counts, on the dense coloured volume with the same origin and voxel_size that holds the blocks from voxel (0, 0, 0) on and reads (0, 0) /
 *   (0, 0, 0, 0) where no block covers a voxel.
 * Coloured target (icp_set_target_tsdf_color_hashed): icp_set_target_tsdf_color's rule -- the SoA planes plus rgba, cr, cg, cb; an
 *   uncoloured hit becomes a hole; *n_points_out is the coloured hits; none: ICP_ERR_NO_TARGET with an empty target.
 * Model loop (icp_track_depth_model_color_hashed): icp_track_depth_model_color's loop with the target from the call above and the
 *   integrate icp_tsdf_integrate_color's on a coloured hashed volume (the touch, growth and room rule).  It accepts colour ICP,
 *   ICP_WEIGHT_COLORS and ICP_METRIC_COLORED; it refuses GICP, null rgbx_frames, source_opt->fix_color_index == 0 and a projective camera
 *   in the params that differs from the depth camera.  Records, statuses and the carried pose of a failed frame are the dense coloured
 *   loop's; host waits are icp_track_depth_model_hashed's.
 * Mesh colours (icp_tsdf_mesh_color_hashed): counts, vertices, normals, triangles and their order are icp_tsdf_mesh_hashed's, bit for bit.
 *   colors_out (max_vertices * 4 bytes, may be NULL) receives one packed colour per vertex: a vertex on the edge v -> v + d takes
 *   icp_tsdf_mesh_color's rule -- both ends have Wc > 0: the lerp of the two at the vertex's t = F_v / (F_v - F_(v+d)); one end has: that
 *   end's colour; neither: zero bytes.  v + d may lie in a neighbouring block.  As a SET of triangles with corner positions, normals and
 *   colours the result equals icp_tsdf_mesh_color's on the dense coloured volume over the blocks' bounding box.
 * Refusals: all four return ICP_ERR_INVALID_ARG with a message that names the call, and touch nothing, without a volume ("no volume"),
 *   on a dense volume ("dense") and on a hashed volume without colours ("no colours").  The four dense-named *_color calls keep refusing
 *   a hashed volume.  The geometry-only hashed calls stay legal on a coloured hashed volume and leave the colours alone.  None of the four
 *   modifies the volume, except the loop's own fusion. */
int icp_tsdf_raycast_color_hashed(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], float* depth_out, float* vertices_out,
                                  float* normals_out, uint8_t* rgba_out, int32_t* n_hits_out, int32_t* n_colored_out);
int icp_set_target_tsdf_color_hashed(icp_ctx* ctx, const icp_depth_camera* cam, const float pose[16], int32_t* n_points_out);
int icp_track_depth_model_color_hashed(icp_ctx* ctx, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames,
                                       const icp_depth_camera* cam, const icp_depth_options* source_opt, const float* gt_frames,
                                       float pose_inout[16], icp_track_frame* out);
int icp_tsdf_mesh_color_hashed(icp_ctx* ctx, float min_weight, int32_t max_vertices, int32_t max_triangles,
                               float* vertices_out, float* normals_out, uint8_t* colors_out, uint32_t* triangles_out,
                               int32_t* n_vertices_out, int32_t* n_triangles_out);

/* -------- direct SDF tracking with a photometric term (an extension): next to its geometric row a pixel adds an intensity row, read from
 * the colour array in the cell the distance is read in (Bylow, Olsson, Kahl, "Direct Camera Pose Tracking and Mapping With Signed Distance
 * Functions", 2014).  DESIGN.md section 6r. --------
 * Where the geometry leaves the pose free (a flat wall) the calls above slide; the texture the volume holds pins it.  Needs the colour array
 * (icp_tsdf_color_create) and the frame's colour frame next to whatever the calls above need.  Target, source, index, params and the
 * convergence reference stay untouched.  tests/sdf_color_restatement.py restates what follows.
 *
 * Sampling: sampled, usable and valid pixels, q, the cell, F, G, r, g, J and w are exactly those above.  A pixel that is not valid there
 *   contributes nothing here either.
 * Intensity field: per corner k of q's cell, in fp32, s_k = (R_k + G_k) + B_k.  S is the nested lerp a + t (b - a) of s along x, then y,
 *   then z; H = (H_x, H_y, H_z) is the analytic gradient of that interpolant per voxel, of G's form with s in place of the distances.
 * Colour validity: a valid pixel is COLOURED iff all eight corners have Wc > 0 and S is finite; n_color counts them.  A valid pixel that
 *   is not coloured contributes its geometric row only.
 * Terms, in fp64 after the conversions, one rounding per operation: I_p = (double)(R + G + B) / 765.0 from the sampled pixel's own bytes
 *   rgbx[4 (v width + u) + 0..2] (colored ICP's intensity); r_c = (double)S / 765.0 - I_p; h = (double)H / (765.0 * (double)voxel_size);
 *   J_c = (q x h, h) with q converted -- J's shape, because both fields are read at the same moved point; w_c = weight^2, with huber > 0
 *   (of icp_sdf_color_options, in intensity units) multiplied by (|r_c| <= huber ? 1 : huber / |r_c|); weight and huber converted from fp32.
 *   `weight` is in metres per unit of intensity, so both residuals are lengths.
 * Sums: 29 doubles.  Entries 0 .. 27 have the layout above for the joint system, each lane term the geometric term + the photometric term
 *   in that order: (w J_i) J_j + (w_c Jc_i) Jc_j, -((w J_i) r) + -((w_c Jc_i) r_c), (w r) r + (w_c r_c) r_c; a pixel that is not coloured
 *   contributes the geometric term alone.  Entry 28 is (w_c r_c) r_c alone.  Counts: {n_depth, n_valid, n_color}.  The fold order is fixed,
 *   without floating-point atomics: bitwise reproducible; against another order each sum differs by at most
 *   (n_valid + n_color) 2^-52 sum (|geometric term| + |photometric term|).
 * Step, stop, failure, statuses and pose composition: those above, unchanged, on the entries 0 .. 26. */
typedef struct icp_sdf_color_options {
    float weight;                    /* metres per unit of intensity, finite and > 0 (a zero weight belongs to the calls above), default 0.1 */
    float huber;                     /* intensity units, finite and >= 0, default 0 = off */
} icp_sdf_color_options;
typedef struct icp_sdf_color_iter {
    int32_t n_valid, n_color, status, pad;   /* as icp_sdf_iter; pad 0 */
    double  cost, cost_color;        /* entry 27 and entry 28 of the sums */
    float   pose[16];
} icp_sdf_color_iter;
typedef struct icp_sdf_color_frame {
    int32_t n_depth, n_valid_first, n_valid_last, n_color_first, n_color_last, iterations, status, pad;
    double  cost_first, cost_last, cost_color_first, cost_color_last;
    float   pose[16];
} icp_sdf_color_frame;
#ifdef __cplusplus
static_assert(sizeof(icp_sdf_color_options) == 8, "icp_sdf_color_options");
static_assert(sizeof(icp_sdf_color_iter) == 96, "icp_sdf_color_iter");
static_assert(sizeof(icp_sdf_color_frame) == 128, "icp_sdf_color_frame");
#endif
int icp_sdf_color_options_default(icp_sdf_color_options* opt);
/* ICP_OK or ICP_ERR_INVALID_ARG; needs neither a context nor a device. */
int icp_sdf_color_options_check(const icp_sdf_color_options* opt);
/* The intensity field and its gradient at n >= 0 world points: s_out n floats (S), grad_out n x 3 floats (H, per voxel), valid_out n bytes:
 * the cell lies inside the volume and its eight Wc > 0 (the geometry's weights play no part); any output may be NULL.  An invalid point
 * reads 0; a NaN is stored as the canonical quiet NaN, as in icp_tsdf_sample. */
int icp_tsdf_sample_color(icp_ctx* ctx, const float* points, int32_t n, float* s_out, float* grad_out, uint8_t* valid_out);
/* The sums of ONE joint step at `pose`: sums_out 29 doubles, counts_out {n_depth, n_valid, n_color}; of opt only stride and huber matter. */
int icp_tsdf_sdf_system_color(icp_ctx* ctx, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const float pose[16],
                              const icp_sdf_options* opt, const icp_sdf_color_options* copt, double* sums_out, int32_t* counts_out);
/* icp_tsdf_align_depth with the photometric term. */
int icp_tsdf_align_depth_color(icp_ctx* ctx, const float* depth, const uint8_t* rgbx, const icp_depth_camera* cam, const icp_sdf_options* opt,
                               const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* rec_out, icp_sdf_color_iter* trace_out);
/* icp_track_depth_sdf with the coloured alignment; integration is always icp_tsdf_integrate_color.  All four calls: ICP_ERR_INVALID_ARG
 * (see icp_last_error) for no volume, no colour array, a null colour frame, bad options of either kind, non-identity depth extrinsics. */
int icp_track_depth_sdf_color(icp_ctx* ctx, const float* depth_frames, const uint8_t* rgbx_frames, int32_t n_frames, const icp_depth_camera* cam,
                              const icp_sdf_options* opt, const icp_sdf_color_options* copt, float pose_inout[16], icp_sdf_color_frame* out);

/* -------- voxelized GICP (an extension): the resident source aligned to a voxel grid of the resident target, without index or search
 * (Koide, Yokozuka, Oishi, Banno, "Voxelized GICP for Fast and Accurate 3D Point Cloud Registration", ICRA 2021).  DESIGN.md section 6s. --------
 * The target is reduced once to a dense grid of cells, each a mean and a normalised sum of plane covariances; a moved source point looks up
 * the ONE cell it falls in and is scored by GICP's plane-to-plane Mahalanobis distance against it.  epsilon and the covariance
 * neighbourhood are the context's icp_gicp_options; the per-point normals are the cached GICP normals of both clouds (icp_get_gicp_normals;
 * covariance_k = 0: the clouds' own normals, which both clouds must then have).  Target, source, index, params, convergence reference and
 * the TSDF volume stay untouched.  tests/vgicp_restatement.py restates what follows.
 *
 * Entering points: a target point enters the grid iff its position and its GICP normal are finite.
 * Cell of a point: per axis c_a = (int)clamp(floorf(p_a / voxel_size), -2^30, 2^30) -- one fp32 division, one rounding; the clamp keeps the
 *   conversion defined for every finite p.
 * Extent: lo_a = min c_a over the entering points, dims_a = max c_a - lo_a + 1; the cell of coordinates c has the index
 *   ((c_z - lo_z) dims_y + (c_y - lo_y)) dims_x + (c_x - lo_x).  dims_x dims_y dims_z <= 2^24, else ICP_ERR_INVALID_ARG with a message that
 *   names the voxel size (the grid is dense).  No entering point: ICP_ERR_NO_TARGET.
 * Integer sums per cell (exact in any order: the build uses integer atomics and keeps its bits): count (int32); sum q_a with
 *   q_a = lrintf(clamp(((p_a - ((float)c_a + 0.5f) voxel_size) / voxel_size) 65536.0f, -32768, 32768)), every fp32 operation rounded once;
 *   sum m_a m_b for (a, b) = xx xy xz yy yz zz with m_a = lrintf(clamp(n_a, -2, 2) 16384.0f) (the clamp changes nothing for a unit normal;
 *   it keeps the products in range for any finite one).  Nine int64 per cell, in that order.
 * Record per cell, fp64 rounded once to fp32, nine floats (mu_x mu_y mu_z S_xx S_xy S_xz S_yy S_yz S_zz):
 *   mu_a = ((double)c_a + 0.5) (double)voxel_size + ((double)sum q_a / (double)count) ((double)voxel_size / 65536.0);
 *   S_ab = (double)sum m_a m_b / (double)(sum m_x m_x + sum m_y m_y + sum m_z m_z): a unit trace, eigenvalues in [0, 1] whatever the
 *   quantisation did, so Sigma below is positive definite for every legal epsilon.  An integer trace of 0 (normals shorter than 2^-15):
 *   S = 0.  An empty cell: count 0, nine zeros.
 * One source point at pose P: p = the fp32 point as icp_transform_points moves it; b = the source's GICP normal as icp_transform_normals
 *   moves it, normalised in fp64 (fp32 components converted, len = sqrt((b_x b_x + b_y b_y) + b_z b_z), b / len).  The point is CONSIDERED
 *   iff its own position is finite.  It is VALID iff it is considered, p is finite, the cell of p lies inside the grid, that cell's count
 *   >= min_points, and b is finite with len > 0.  Then in fp64, one rounding per operation: r = mu - p;
 *   Sigma_aa = 2 - (1 - eps)(S_aa + b_a b_a), Sigma_ab = -((1 - eps)(S_ab + b_a b_b)), eps converted from fp32; M = adj(Sigma) / det(Sigma)
 *   entry by entry as GICP's; J = [A | I] with A = -[p]x; N = (double)count.
 * Sums: 28 doubles in icp_tsdf_sdf_system's layout: N (J^T M J)_ij for j >= i at i 6 - i (i - 1) / 2 + (j - i); N (J^T M r)_i at 21 + i;
 *   N r^T M r at 27.  Counts: {considered, valid}.  Folded in a fixed order without floating-point atomics: bitwise reproducible; against
 *   another summation order each sum differs by at most n_valid 2^-52 sum |term|.
 * Step, stop and failure are direct SDF tracking's (above) on these sums: a step fails with fewer than min_valid valid points or a
 *   non-finite solution; otherwise the point-to-plane solve and the fp32 composition dT pose; the stop test is made on the solved six-vector
 *   after a successful step; what is still enqueued behind the end returns at once, and nothing crosses to the host between iterations.
 *   A failed alignment returns the pose it started with and ICP_ERR_NO_CORRESPONDENCES (ICP_ERR_NO_SOURCE when no point is considered). */
typedef struct icp_vgicp_options {
    float   voxel_size;              /* metres, finite and > 0, default 0.25 */
    int32_t min_points;              /* >= 1, default 1: a cell with fewer target points scores nothing */
    int32_t n_iterations;            /* 1 .. 1000, default 30 */
    int32_t min_valid;               /* >= 6, default 64 */
    float   stop_rotation, stop_translation;   /* >= 0, default 1e-5 each; either at 0 turns the stop off */
} icp_vgicp_options;
typedef struct icp_voxel_grid_info {
    int32_t lo[3], dims[3];          /* the extent in cells */
    int32_t n_occupied, n_points;    /* cells with count > 0; target points that entered */
} icp_voxel_grid_info;
/* The records are direct SDF tracking's, field for field: n_depth counts the CONSIDERED points, n_valid_* the valid ones. */
typedef icp_sdf_iter icp_vgicp_iter;
typedef icp_sdf_frame icp_vgicp_record;
#ifdef __cplusplus
static_assert(sizeof(icp_vgicp_options) == 24, "icp_vgicp_options");
static_assert(sizeof(icp_voxel_grid_info) == 32, "icp_voxel_grid_info");
#endif
int icp_vgicp_options_default(icp_vgicp_options* opt);
/* ICP_OK or ICP_ERR_INVALID_ARG; needs neither a context nor a device. */
int icp_vgicp_options_check(const icp_vgicp_options* opt);
/* Builds the grid of the resident target at opt->voxel_size (computing the target's GICP normals if their cache is cold) and keeps it in
 * the context; info_out is optional.  Whatever drops the target's GICP normal cache drops the grid: every call that replaces the target,
 * and icp_set_gicp_options.  A grid that is current for this voxel size is not rebuilt. */
int icp_voxelize_target(icp_ctx* ctx, const icp_vgicp_options* opt, icp_voxel_grid_info* info_out);
/* The grid icp_voxelize_target (or an alignment) left: counts_out one int32 per cell, sums_out nine int64 per cell, cells_out nine floats
 * per cell; any pointer may be NULL.  ICP_ERR_INVALID_ARG without a current grid. */
int icp_get_voxel_grid(icp_ctx* ctx, int32_t* counts_out, int64_t* sums_out, float* cells_out);
/* The sums of ONE step of the resident source at `pose`: sums_out 28 doubles, counts_out {considered, valid}; of opt only voxel_size and
 * min_points matter (the others must still be legal).  Builds the grid if there is none for this voxel size. */
int icp_vgicp_system(icp_ctx* ctx, const float pose[16], const icp_vgicp_options* opt, double* sums_out, int32_t* counts_out);
/* Aligns the resident source to the grid from pose_inout: builds the grid if there is none or voxel_size changed, enqueues n_iterations x
 * (accumulate, solve) at once, stops on the device and reads ONE record back.  rec_out is optional; trace_out: NULL, or max_trace records,
 * of which min(max_trace, n_iterations) are written, those past the last step tried zeroed.  Returns the record's status.  Refuses with a
 * reason (icp_last_error): no target (ICP_ERR_NO_TARGET), no source (ICP_ERR_NO_SOURCE), bad options, covariance_k = 0 with a cloud
 * that has no normals, a grid of more than 2^24 cells (ICP_ERR_INVALID_ARG). */
int icp_vgicp_align(icp_ctx* ctx, const icp_vgicp_options* opt, float pose_inout[16], icp_vgicp_record* rec_out, icp_vgicp_iter* trace_out,
                    int32_t max_trace);

/* -------- scan-to-map laser tracking (an extension): a persistent voxel map that scans are aligned to and fused into.  DESIGN.md section 6t. --------
 * The laser counterpart of the TSDF volume: voxelized GICP's grid of cells (above) as state of the context with a FIXED extent, which the
 * resident target or source is fused into at a pose, and which the resident source is aligned to in place of the target's grid.  The
 * per-cell state is the count and the nine integer sums above, so the map after any set of inserts depends neither on their order nor on
 * the order of the points within one, and keeps its bits.  The map and the target's grid are separate state: nothing above changes what it
 * returns.  The map holds sums, not normals: it survives icp_set_target, icp_set_source and icp_set_gicp_options.
 * tests/vmap_restatement.py restates what follows.
 *
 * Extent: lo in cell coordinates by the rule above (c_a = (int)clamp(floorf(p_a / voxel_size), -2^30, 2^30)), dims_a >= 1 cells per axis,
 *   dims_x dims_y dims_z <= 2^24 (the map is dense); voxel_size finite and > 0.  Anything else: ICP_ERR_INVALID_ARG with a reason.  The
 *   cell of coordinates c has the index ((c_z - lo_z) dims_y + (c_y - lo_y)) dims_x + (c_x - lo_x).
 * Insert of a cloud at a pose P.  The normals are the cloud's GICP normals under the context's icp_gicp_options, as above (covariance_k =
 *   0: its own, which it must then have).  A point is CONSIDERED iff its own position is finite.  It ENTERS iff, in addition,
 *   p' = icp_transform_points(P, p) (fp32, ((P_r0 x + P_r1 y) + P_r2 z) + P_r3) and n' = icp_transform_normals(P, n) (the fp32 normal
 *   matrix of the pose) are both finite.  An entering point is quantised exactly as a target point is above, with p' and n' in place of p
 *   and n: the cell, q_a, m_a and every clamp; n' is not renormalised.  If its cell lies inside the extent the cell's count goes up by one
 *   and its nine sums by the point's nine integers; otherwise the point is OUTSIDE and dropped.
 * Records: after an insert the record of every cell with count > 0 is the function of its sums and count given above (fp64 rounded once
 *   to fp32; S over the integer trace, S = 0 for a zero trace); an empty cell holds nine zeros.
 * Align: the sums, counts, step, stop, records and failure rules of icp_vgicp_system / icp_vgicp_align, with the map's cells in place of
 *   the grid's.  opt->voxel_size must equal the map's.  A source and a map are needed, a target is not. */
typedef struct icp_voxel_map_options {
    float   voxel_size;              /* metres, finite and > 0 */
    int32_t lo[3], dims[3];          /* the extent in cells: lowest cell, cells per axis (each >= 1, product <= 2^24) */
} icp_voxel_map_options;
typedef struct icp_voxel_map_insert_info {
    int32_t n_considered, n_entered, n_outside;   /* points of this insert: finite position; finite p' and n' as well; of those, outside the extent */
    int32_t n_cells_touched, n_cells_new;         /* cells this insert added to; of those, cells whose count was 0 before it */
    int32_t n_occupied;                           /* cells with count > 0 after it: the running total */
} icp_voxel_map_insert_info;
typedef struct icp_voxel_map_info {
    float   voxel_size;
    int32_t lo[3], dims[3];
    int32_t n_occupied;
} icp_voxel_map_info;
#ifdef __cplusplus
static_assert(sizeof(icp_voxel_map_options) == 28, "icp_voxel_map_options");
static_assert(sizeof(icp_voxel_map_insert_info) == 24, "icp_voxel_map_insert_info");
static_assert(sizeof(icp_voxel_map_info) == 32, "icp_voxel_map_info");
#endif
/* ICP_OK or ICP_ERR_INVALID_ARG; needs neither a context nor a device. */
int icp_voxel_map_options_check(const icp_voxel_map_options* opt);
/* Allocates the map (per cell 4 + 72 + 40 bytes of state and a 4-byte stamp) and clears it.  A second create replaces the map. */
int icp_voxel_map_create(icp_ctx* ctx, const icp_voxel_map_options* opt);
/* Frees the map (ICP_OK without one). */
int icp_voxel_map_destroy(icp_ctx* ctx);
/* Fuses the resident target (which = 0) or source (which = 1) into the map at `pose`; info_out is optional (without it the host reads
 * nothing back).  Only the records of the cells the insert touched are recomputed.  ICP_ERR_INVALID_ARG without a map, for which outside
 * {0, 1}, for covariance_k = 0 with a cloud that has no normals; ICP_ERR_NO_TARGET / ICP_ERR_NO_SOURCE without the cloud. */
int icp_voxel_map_insert(icp_ctx* ctx, int32_t which, const float pose[16], icp_voxel_map_insert_info* info_out);
/* The map: counts_out one int32 per cell, sums_out nine int64 per cell, cells_out nine floats per cell; any pointer may be NULL.
 * ICP_ERR_INVALID_ARG without a map, and for a hashed map (icp_get_voxel_map_hashed). */
int icp_get_voxel_map(icp_ctx* ctx, icp_voxel_map_info* info_out, int32_t* counts_out, int64_t* sums_out, float* cells_out);
/* Replaces the integer state (counts >= 0: one int32 per cell; sums: nine int64 per cell) and recomputes every record and n_occupied.
 * Dense maps only (a hashed map: icp_voxel_map_upload_hashed). */
int icp_voxel_map_upload(icp_ctx* ctx, const int32_t* counts, const int64_t* sums);
/* icp_vgicp_system against the map. */
int icp_voxel_map_system(icp_ctx* ctx, const float pose[16], const icp_vgicp_options* opt, double* sums_out, int32_t* counts_out);
/* icp_vgicp_align against the map.  Refuses with a reason: no map, opt->voxel_size other than the map's, bad options (ICP_ERR_INVALID_ARG),
 * no source (ICP_ERR_NO_SOURCE), covariance_k = 0 with a source that has no normals. */
int icp_voxel_map_align(icp_ctx* ctx, const icp_vgicp_options* opt, float pose_inout[16], icp_vgicp_record* rec_out, icp_vgicp_iter* trace_out,
                        int32_t max_trace);
/* Tracking: scan 0 (xyz[0]: n[0] x 3 floats, normals[0] likewise) becomes the source, as icp_set_source(xyz, normals, NULL, n) makes it, and
 * is inserted at pose_inout; scan k >= 1 becomes the source and is aligned from the current pose; on ICP_OK it is inserted at the pose
 * found (out[k - 1] its record).  A failed scan carries the pose, is not inserted, records its status, and tracking goes on; the first
 * error in scan order is returned.  normals, or normals[k], may be NULL when the context's covariance_k > 0.  The host reads one record per
 * scan.  The last scan stays resident as the source.  out: n_scans - 1 records (may be NULL for n_scans = 1). */
int icp_track_scans_vmap(icp_ctx* ctx, const float* const* xyz, const float* const* normals, const int32_t* n, int32_t n_scans,
                         const icp_vgicp_options* opt, float pose_inout[16], icp_vgicp_record* out);

/* -------- the hashed voxel map (an extension): the same map without an extent.  DESIGN.md section 6u. --------
 * A second storage for the voxel map above.  The per-cell state, the options and every rule of an insert, of the records and of an
 * alignment are the ones above, word for word; the cells are addressed by a hash of their coordinates instead of by their place in a box.
 * The entry points above (icp_voxel_map_insert / _system / _align / _destroy, icp_track_scans_vmap) work on whichever map the context
 * holds; with a dense map they do exactly what they did.  tests/hmap_restatement.py restates what follows.
 *
 * Key: a cell of coordinates c is STORABLE iff -2^20 <= c_a < 2^20 on every axis; its key is
 *   ((uint64)(c_z + 2^20) << 42) | ((uint64)(c_y + 2^20) << 21) | (uint64)(c_x + 2^20).  An empty slot holds ~0ull, which is never a key.
 *   An entering point whose cell is not storable is OUTSIDE (n_outside), as beyond a dense extent; a source point whose cell is not
 *   storable is not valid.
 * Table: capacity is a power of two, 2^8 .. 2^26 slots.  The home slot of a key is (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2
 *   capacity); collisions go to the next slot, wrapping at the end (linear probing); every probe loop is bounded by capacity.  An insert
 *   claims a slot with a 64-bit atomicCAS(empty -> key) and accepts a slot that already holds its key.  WHERE a cell is stored is not part
 *   of the contract; the set of (key, count, sums, record) is, exactly: it equals a dense map's over a covering extent bit for bit.
 * Room rule: before a cloud of n points goes in, the host makes sure that capacity >= 2 (n_occupied + n), with n_occupied exact or the
 *   host's upper bound on it (the last value read plus the points of every insert since); where the bound fails the true count is read,
 *   and where that fails the table is doubled until it holds.  Past 2^26 slots the call is refused (ICP_ERR_INVALID_ARG, with a reason)
 *   before anything is modified.  So an insert always finds room and probe chains stay short.  Points that found no slot are counted all
 *   the same (n_unplaced, which stays 0); a nonzero value makes the call return ICP_ERR_HIP with a message.
 * Growth: rehashing allocates and clears a larger table and re-inserts every occupied slot's key, copying its count, sums and record; the
 *   set of (key, state) is unchanged bit for bit.  n_grown counts the times the table was enlarged.  A table never shrinks.
 * A capacity that is not a power of two is rounded UP to one (and to 2^8 at least). */
typedef struct icp_voxel_hash_map_info {
    float   voxel_size;
    int32_t capacity, n_occupied, n_grown, n_unplaced, reserved[3];
} icp_voxel_hash_map_info;
#ifdef __cplusplus
static_assert(sizeof(icp_voxel_hash_map_info) == 32, "icp_voxel_hash_map_info");
#endif
/* Allocates and clears a hashed map of at least `capacity` slots (8 + 4 + 72 + 40 + 4 bytes per slot); replaces any map, dense or hashed.
 * ICP_ERR_INVALID_ARG: voxel_size not finite and > 0, capacity < 1 or > 2^26. */
int icp_voxel_map_create_hashed(icp_ctx* ctx, float voxel_size, int32_t capacity);
/* Rehashes into a table of at least `capacity` slots; a smaller or equal capacity is a no-op.  Hashed maps only; capacity in 1 .. 2^26.
 * On a pruned map with vacated slots the rehash is a compaction (below). */
int icp_voxel_map_reserve(icp_ctx* ctx, int32_t capacity);
/* The occupied entries sorted by key ascending (z, then y, then x): coords_out three int32 per entry, counts_out one, sums_out nine int64,
 * cells_out nine floats; any pointer may be NULL.  ICP_ERR_INVALID_ARG without a hashed map, or for max_entries < n_occupied while an
 * array is asked for.  A save path: the host downloads the slots, compacts and sorts them.  A slot that a prune vacated (below) is no
 * entry: only cells with count > 0 are returned. */
int icp_get_voxel_map_hashed(icp_ctx* ctx, icp_voxel_hash_map_info* info_out, int32_t max_entries, int32_t* coords_out, int32_t* counts_out,
                             int64_t* sums_out, float* cells_out);
/* Replaces the map's state by n entries (coords: three int32 each; counts >= 0; sums: nine int64 each) and computes every record; an
 * entry with count 0 is an empty cell and is not stored.  The capacity is kept, or grown so that capacity >= 2 n.  Refused with a
 * reason before anything is modified: n < 0, a negative count, a coordinate that is not storable, a coordinate that occurs twice, n
 * beyond 2^25. */
int icp_voxel_map_upload_hashed(icp_ctx* ctx, int32_t n, const int32_t* coords, const int32_t* counts, const int64_t* sums);

/* -------- a local map (an extension): forgetting the cells beyond a radius.  DESIGN.md section 6v. --------
 * A cell is a count and nine integer sums, so REMOVING a cell is putting it back into the cleared state bit for bit: count 0, nine sums
 * 0, an all-zero 40-byte record, stamp 0 -- exactly what icp_voxel_map_create leaves.  A pruned map therefore equals, exactly, a map
 * that the removed cells' points never went into.  tests/vmap_prune_restatement.py restates what follows.
 *
 * Rule of prune(centre, radius): it applies to every cell with count > 0.  With c the cell's coordinates (dense: lo + its index per axis;
 *   hashed: from the key), in fp32, operation for operation, without contraction:
 *     d_a = ((float)c_a + 0.5f) * voxel_size - centre_a  (a = x, y, z),   d2 = (d_x d_x + d_y d_y) + d_z d_z,
 *   the cell is KEPT iff d2 <= r2, with r2 = radius * radius computed once on the host in fp32; an infinite r2 keeps everything.  Every
 *   other cell with points is removed.  centre must be finite, radius finite and >= 0: otherwise ICP_ERR_INVALID_ARG with a reason, before
 *   anything is modified; without a map the call is refused likewise.
 * Hashed storage: a removed cell KEEPS its key and loses its content -- a VACATED slot.  Keys still only go from empty to a key, probes
 *   pass the slot, a source point that falls in it reads n = 0 < min_points and is not valid, and a later insert into that cell finds the
 *   key, sees the count's old value 0 and counts a new cell (n_cells_new, n_occupied), as the dense map does.  n_vacated counts the slots
 *   vacated since the last compaction; a slot that is occupied again stays counted, so it is an upper bound on the keyed slots without
 *   points.  The room rule becomes capacity >= 2 (n_occupied + n_vacated + n).  Where it fails with n_vacated = 0 the table grows as
 *   before.  Where it fails with n_vacated > 0 the table is COMPACTED: rehashed without the slots that have no points, into the
 *   smallest power of two >= capacity for which 2 (n_occupied + n) <= 0.75 capacity (the 0.75 is hysteresis: a map that sits just under
 *   the limit is not rebuilt on every scan); then n_vacated = 0 and n_compacted goes up; n_grown goes up when the capacity did.  Past
 *   2^26 slots the call is refused as before.  icp_voxel_map_reserve to a larger capacity compacts on the way when n_vacated > 0;
 *   icp_get_voxel_map_hashed returns the entries with count > 0; icp_voxel_map_upload_hashed and a second create reset n_vacated.
 * A context that never prunes does exactly what it did. */
typedef struct icp_voxel_map_prune_info {
    int32_t n_removed;         /* cells this call emptied */
    int32_t n_occupied;        /* cells with count > 0 after it */
    int32_t n_vacated;         /* hashed: slots vacated since the last compaction (after the call); dense: 0 */
    int32_t n_compacted;       /* hashed: compactions over the map's life; dense: 0 */
    int32_t capacity;          /* hashed: slots; dense: cells of the extent */
    int32_t reserved;
    int64_t n_points_removed;  /* the sum of the removed cells' counts */
} icp_voxel_map_prune_info;
#ifdef __cplusplus
static_assert(sizeof(icp_voxel_map_prune_info) == 32, "icp_voxel_map_prune_info");
#endif
/* Removes every cell of the map (dense or hashed) whose centre lies beyond `radius` of `centre`, by the rule above.  info_out may be NULL:
 * then the call is enqueued and the host waits for nothing. */
int icp_voxel_map_prune(icp_ctx* ctx, const float centre[3], float radius, icp_voxel_map_prune_info* info_out);
/* Hashed maps only: drops the vacated slots at the current capacity (a no-op with none); the entries keep their bits.  For save paths
 * and tests; the room rule compacts by itself. */
int icp_voxel_map_compact(icp_ctx* ctx);
/* icp_track_scans_vmap with a local map: after every insert, scan 0 included, the map is pruned about the translation of the pose the
 * scan was inserted at, with keep_radius (finite and > 0).  A scan that fails is carried and skipped as there: no insert, no prune, and
 * its prune_out entry is all zero.  prune_out: n_scans entries, or NULL.  The host still waits once per scan: a prune's info comes back
 * with the next scan's record, the last one with the closing wait. */
int icp_track_scans_vmap_local(icp_ctx* ctx, const float* const* xyz, const float* const* normals, const int32_t* n, int32_t n_scans,
                               const icp_vgicp_options* opt, float keep_radius, float pose_inout[16], icp_vgicp_record* out,
                               icp_voxel_map_prune_info* prune_out);

/* PointCloud(pcl::PointCloud<PointXYZ>::Ptr) (PointCloud.h:41-76): normals of an unorganised scan from its k nearest
 * neighbours (pcl::NormalEstimation, setKSearch(5), viewpoint (0,0,0)): exact k-NN on the device, fp64 PCA, normal flipped
 * towards the viewpoint.  k in {3..8} (else ICP_ERR_INVALID_ARG).  Non-finite points, and every point of a cloud with fewer than
 * 3 finite points, get NaN normals and curvature; fewer than k finite points: all of them are the neighbours; coincident
 * neighbours (zero covariance): (+-1, 0, 0) flipped, curvature 0.  curvature_out may be NULL.  Uses scratch
 * buffers of the context only (target / source stay untouched). */
int icp_estimate_normals(icp_ctx* ctx, const float* xyz, int32_t n, int32_t k, const float viewpoint[3], float* normals_out, float* curvature_out);

/* The selection predicate of RANDOM_SAMPLING: point `index` is kept in resample number `iteration` iff the returned
 * 32-bit hash is < proba * 2^32.  Exposed so host code (and the test oracle) can reproduce the device's choice exactly. */
uint32_t icp_select_hash(uint32_t seed, uint32_t iteration, uint32_t index);

/* -------- global registration (an extension): FPFH features, feature matching, RANSAC --------
 * ICP is local; these entry points find initial poses for it from the two resident clouds alone (both need normals): Fast Point
 * Feature Histograms (Rusu, Blodow, Beetz, ICRA 2009), an exact nearest neighbour in feature space, RANSAC over three-point
 * hypotheses.  The winners go to icp_run_multistart.  Nothing else in the library changes behaviour.
 *
 * Features, once per cloud and cached (a new target / source, a depth upload of that cloud, or new options drop the cache):
 *   neighbourhood  the k smallest (fp32 d^2 = (dx^2 + dy^2) + dz^2, index) pairs over the cloud's finite points, the point itself
 *                  included -- icp_estimate_normals' rule; k in {5, 10, 20}; fewer than k finite points: all of them.  Stored per point
 *                  in ascending (d^2, index) order; unfilled slots are (-1, +inf); a non-finite point has none.
 *   pair features  of point p and each neighbour q with d^2 > 0, in fp64 from the fp32 coordinates and normals: dp = q - p, f4 = |dp|,
 *                  a1 = n_p.dp / f4, a2 = n_q.dp / f4; if |a1| < |a2| the pair is taken from q's side (the normals swapped, dp <- -dp,
 *                  f3 = -a2), otherwise f3 = a1; v = dp x n1, the pair skipped when |v| = 0 or an input is not finite; v <- v / |v|,
 *                  w = n1 x v, f1 = v.n2, f2 = atan2(w.n2, n1.n2).  (Dot products and squared norms add as (x + y) + z.)
 *   bins           11 per feature, floor(11 (x - lo) / (hi - lo)) clamped to 0..10, over [-1, 1] (f1), [-pi, pi] (f2), [-1, 1] (f3).
 *   SPFH           33 integer counts per point (uint8: bins of f1, f2, f3) and the number of contributing pairs, for EVERY point.
 *   FPFH           h(p) = SPFH(p) / max(pairs(p), 1);  F(p) = h(p) + sum_i w_i h(q_i) over the neighbours with d_i > 0 in stored order,
 *                  w_i = (1 / d_i) / sum_j (1 / d_j), d = sqrt(d^2) in fp64; fp64 sums, one rounding to fp32.  33 NaNs for a point with a
 *                  non-finite position or normal or with no contributing pair: such a row takes no part in matching.
 *   keypoints      the points whose index is a multiple of feature_stride (PointCloud.h:325-343's stride idiom): FPFH, matching and RANSAC
 *                  use keypoints only, neighbourhoods and SPFH the whole cloud.  Keypoint r is point r * feature_stride.
 * Matching: for every source keypoint the target keypoint with the smallest d = sum over the 33 bins, in order, of (a_b - c_b)^2 (fp32, one
 *   rounding per operation); ties: the lowest target index; NaN rows never match and are never matched.  mutual = 1: pair (i, j) is kept
 *   only if i is also the match of j in the other direction.  The M pairs are listed in ascending source order.
 * RANSAC: hypothesis h (0 .. n_hypotheses - 1) draws c_j = icp_select_hash(seed, h, j) mod M, j = 0, 1, 2.  Its status is, in this order,
 *   ICP_GLOBAL_REPEATED   two draws are equal;
 *   ICP_GLOBAL_EDGES      for one of the edges (0,1), (1,2), (2,0): min(l_src, l_tgt) < edge_similarity max(l_src, l_tgt), fp64 lengths;
 *   ICP_GLOBAL_DEGENERATE on either side |e1 x e2|^2 <= 1e-6 |e1|^2 |e2|^2, e1 = p1 - p0, e2 = p2 - p0 in fp64 (collinear within 1e-3 rad),
 *                         or a pose that is not finite;
 *   ICP_GLOBAL_VALID      else: the three-point Kabsch fit in fp64 (unweighted centroids, R = U diag(1, 1, det(U V^T)) V^T, t = tm - R sm),
 *                         rounded once to fp32.
 *   A valid hypothesis is scored over all M pairs: the source point moved by the fp32 pose (((R_i0 x + R_i1 y) + R_i2 z) + t_i),
 *   d^2 = (dx^2 + dy^2) + dz^2 in fp32, an inlier when d^2 <= inlier_distance^2 (squared once in fp32); n_inliers and the fp64 sum of the
 *   inliers' d^2, reduced in a fixed order (two runs agree bit for bit).  Ranking of the valid ones: more inliers, then the smaller sum,
 *   then the lower h. */
enum { ICP_CLOUD_TARGET = 0, ICP_CLOUD_SOURCE = 1, ICP_CLOUD_BOTH = 2 };
enum { ICP_GLOBAL_VALID = 0, ICP_GLOBAL_REPEATED = 1, ICP_GLOBAL_EDGES = 2, ICP_GLOBAL_DEGENERATE = 3 };
typedef struct icp_global_options {
    int32_t k;                /* neighbours per point, 5, 10 or 20                       default 20   */
    int32_t feature_stride;   /* keypoints: every feature_stride-th point, >= 1          default 1    */
    int32_t mutual;           /* 1: keep mutual matches only                             default 1    */
    int32_t n_hypotheses;     /* 1 .. 65536                                              default 4096 */
    float   edge_similarity;  /* 0 .. 1                                                  default 0.9  */
    float   inlier_distance;  /* metres (NOT squared), > 0                               default 0.005 */
    uint32_t seed;            /*                                                         default 0    */
    int32_t n_best;           /* poses icp_register_global returns, 1 .. 256             default 16   */
} icp_global_options;
typedef struct icp_global_hypothesis {
    float   pose[16];         /* column-major; identity unless status == ICP_GLOBAL_VALID */
    int32_t n_inliers;
    int32_t reserved;         /* 0 (keeps the double on an 8-byte boundary with no hidden padding: records compare byte for byte) */
    double  sum_d2;           /* of the inliers' fp32 d^2 */
    int32_t status;           /* ICP_GLOBAL_* */
    int32_t draw[3];          /* the three correspondences drawn (positions in icp_match_features' list) */
} icp_global_hypothesis;
int icp_global_options_default(icp_global_options* o);
int icp_set_global_options(icp_ctx* ctx, const icp_global_options* o);      /* NULL: the defaults; out of range: ICP_ERR_INVALID_ARG */
int icp_get_global_options(const icp_ctx* ctx, icp_global_options* o);
/* Computes (or finds cached) the features of the target, the source or both (ICP_CLOUD_*).  A cloud without normals:
 * ICP_ERR_INVALID_ARG. */
int icp_compute_features(icp_ctx* ctx, int32_t which);
/* which = ICP_CLOUD_TARGET or ICP_CLOUD_SOURCE below.  Each computes what is not cached, copies min(max_points, n) rows and sets *n_out
 * to n: the number of keypoints (features: n x 33 floats row-major, row r = point r * feature_stride) or of points (SPFH: n x 33 counts
 * and n pair counts; neighbours: n x k indices and n x k d^2).  Output pointers may be NULL with max_points = 0. */
int icp_get_features(icp_ctx* ctx, int32_t which, float* out, int32_t max_points, int32_t* n_out);
int icp_get_spfh(icp_ctx* ctx, int32_t which, uint8_t* counts, int32_t* pairs, int32_t max_points, int32_t* n_out);
int icp_get_feature_neighbours(icp_ctx* ctx, int32_t which, int32_t* idx, float* d2, int32_t max_points, int32_t* n_out);
/* The correspondences (original point indices), ascending in src_idx; *m_out = M.  M = 0 is not an error here. */
int icp_match_features(icp_ctx* ctx, int32_t* src_idx, int32_t* tgt_idx, int32_t max_pairs, int32_t* m_out);
/* Features, matching, RANSAC.  poses_out: n_best x 16 floats (column-major poses, best first); best_out (optional): their records;
 * *n_out: how many there are (min(n_best, valid hypotheses)).  Fewer than 3 correspondences, or no valid hypothesis:
 * ICP_ERR_NO_CORRESPONDENCES with *n_out = 0 -- reported, never a hang. */
int icp_register_global(icp_ctx* ctx, float* poses_out, icp_global_hypothesis* best_out, int32_t* n_out);
/* Every hypothesis of the last icp_register_global, in order of h. */
int icp_get_global_hypotheses(const icp_ctx* ctx, icp_global_hypothesis* out, int32_t max_out, int32_t* count_out);

/* -------- bilateral depth filter: KinectFusion's first stage, in front of every tracker that aligns a depth frame --------
 * Off by default (radius 0): nothing changes.  With radius > 0 every depth frame a call takes is filtered on the device right after its
 * upload, into a second buffer, and the consumers that ALIGN a frame read the filtered one: the depth clouds (icp_set_target_depth,
 * icp_set_source_depth, icp_track_depth_frames, the source of every icp_track_depth_model*), and the direct SDF calls (icp_tsdf_sdf_system,
 * icp_tsdf_align_depth, icp_track_depth_sdf and their _color forms).  The consumers that FUSE or EXPORT a frame keep reading the raw one:
 * every integrate (dense and hashed, geometric and coloured, the hashed touch and allocation included), icp_depth_mesh and
 * icp_backproject_depth.  Colour frames are never filtered.
 *
 * Contract (fp32, the operations in the order written, one rounding each; the device evaluates no exp):
 *   Tables, computed in fp64 and rounded once: S[(dy + r)(2r + 1) + (dx + r)] = (float)exp(-(dx^2 + dy^2) / (2 sigma_space^2));
 *   R[q] = (float)exp(-4.5 (q + 0.5) / 256), q = 0 .. 255 (the cut-off is 3 sigma_range, so R does not depend on the options);
 *   inv_bin = (float)(256 / (9 sigma_range^2)).
 *   A depth is USABLE iff it is finite and > 0.  Pixel (u, v) with centre c: c not usable -> the output is c unchanged (holes stay holes;
 *   MINF, NaN, +inf, 0 and negatives pass through).  Else num = 0, den = 0; for dy = -r .. r (outer), dx = -r .. r (inner): skip a
 *   neighbour outside the image; n = its depth, skip unless usable; D = n - c; e = D * D; t = e * inv_bin; skip unless t < 256.0f (which
 *   also rejects inf and NaN); q = (int)t; w = S[..] * R[q]; num = num + w * n; den = den + w.  The output is num / den (the centre always
 *   enters with q = 0, so den > 0).  Nothing is filled in, and nothing beyond 3 sigma_range of the centre bleeds across a depth edge. */
typedef struct icp_depth_filter_options {
    int32_t radius;        /* 0 = off (default); 1..4: window (2r+1)^2 */
    float   sigma_space;   /* pixels, > 0, default 4.5 */
    float   sigma_range;   /* metres, > 0, default 0.03 */
} icp_depth_filter_options;
enum { ICP_DEPTH_FILTER_MAX_RADIUS = 4, ICP_DEPTH_FILTER_RANGE_BINS = 256,
       ICP_DEPTH_FILTER_TILE_W = 32, ICP_DEPTH_FILTER_TILE_H = 8 };   /* the kernel's tile of pixels per block (tests choose shapes around it) */
int icp_depth_filter_options_default(icp_depth_filter_options* opt);
/* ICP_OK or ICP_ERR_INVALID_ARG (a radius outside 0 .. 4, a non-finite or non-positive sigma, a sigma_range whose inv_bin is not finite);
 * needs neither a context nor a device. */
int icp_depth_filter_options_check(const icp_depth_filter_options* opt);
int icp_set_depth_filter_options(icp_ctx* ctx, const icp_depth_filter_options* opt);   /* NULL = defaults (off) */
int icp_get_depth_filter_options(const icp_ctx* ctx, icp_depth_filter_options* opt);
/* The tables the device will use for `opt`: spatial_out (2r + 1)^2 floats (none with radius 0), range_out 256 floats, *inv_bin_out; any
 * output may be NULL.  Needs neither a context nor a device. */
int icp_depth_filter_tables(const icp_depth_filter_options* opt, float* spatial_out, float* range_out, float* inv_bin_out);
/* Filters one frame, host to host, with `opt` (NULL: the context's options); radius 0 copies the input.  depth_out: width x height floats. */
int icp_filter_depth(icp_ctx* ctx, const float* depth, int32_t width, int32_t height, const icp_depth_filter_options* opt, float* depth_out);

/* -------- a laser scan into the TSDF volume: icp_tsdf_integrate_cloud --------
 * Every integrate above takes a depth image and a pinhole camera.  This one takes a RESIDENT cloud, unorganised, in icp_voxel_map_insert's
 * convention (which = 0: the target, 1: the source), and fuses it as ONE observation, as one depth frame is: every usable point is a ray
 * from the sensor centre, walked through the truncation band in steps of one voxel, and each sample observes its nearest voxel.  It works
 * on whichever volume the context holds, dense (icp_tsdf_create) or hashed (icp_tsdf_create_hashed); everything that reads the volume
 * (icp_tsdf_sample, the ray-casts, icp_tsdf_mesh / icp_tsdf_mesh_hashed, evict and insert) takes the result as it takes fused frames.
 * On a COLOURED volume the call writes geometry only: the colour array or pool is neither read nor written.  The scan's colours go in
 * with icp_tsdf_integrate_cloud_color (below).
 * Unless carving is on (icp_set_tsdf_carve_options below, a step of its own, off by default) the call carves NO free space in front of
 * the band (as the hashed depth touch allocates none there): a voxel nearer to the sensor than range - truncation is not observed.  A ray writes a line ONE voxel wide, so a surface becomes watertight only where neighbouring beams
 * are closer than a voxel at the surface: choose voxel_size for the scanner's angular step and the range of interest.
 * The result does not depend on the order of the points, nor on any race: the scan is accumulated per voxel in integers (S 64-bit, N
 * 32-bit, two plain arrays: no limit on the size of the cloud beyond int32 points) and folded into the float state once.  The
 * accumulators cost 12 bytes per voxel (6 KiB per pool block of a hashed volume, 1.5 x a dense volume), are allocated at the first call
 * and leave with the volume.
 *
 * Contract (fp32, one rounding per operation, in the order written; tests/tsdf_cloud_restatement.py restates it in numpy).  P = pose (scan
 * frame -> world, column-major, P_rc = pose[4 c + r]), e = sensor_origin (the ray origin in the scan frame; NULL = (0, 0, 0)), o, s,
 * truncation, max_weight and max_depth the volume's options (min_depth and ray_step are not used).
 *   Sensor centre: c_r = (P_r0 e_x + (P_r1 e_y + P_r2 e_z)) + P_r3.
 *   Ray of point p (finite on all three axes, else not usable): w_r = (P_r0 p_x + (P_r1 p_y + P_r2 p_z)) + P_r3; d = w - c per axis;
 *   r2 = d_x d_x + (d_y d_y + d_z d_z); r = sqrtf(r2); usable iff r is finite, r > 0 and r <= max_depth; u = d / r per axis.
 *   Samples m = 0 .. M, M = ceil(2 truncation / s) in double (the hashed touch's walk): t_m = fminf((r - truncation) + (float)m s,
 *   r + truncation), skipped unless t_m > 0; q_a = c_a + t_m u_a; the sample's voxel is the nearest one, g_a = floorf(((q_a - o_a) / s) +
 *   0.5f).  In range iff, tested in float before any cast, -2^23 <= g_a <= 2^23 - 1 on every axis (hashed) or 0 <= g_a <= n_a - 1 (dense);
 *   any other sample is counted in n_outside and does nothing.  An in-range sample whose voxel equals that of the ray's previous in-range
 *   sample is skipped; every other in-range sample is counted in n_samples.
 *   Observation of voxel g by that sample: x_a = o_a + (float)g_a s; e_a = x_a - c_a; proj = e_x u_x + (e_y u_y + e_z u_z); sdf = r - proj;
 *   skipped if sdf < -truncation; f = fminf(1, sdf / truncation); k = (int)rintf(f * 32768.f); the voxel's S += k, N += 1.
 *   Fold, for every voxel with N > 0: fbar = (float)((double)S / ((double)N * 32768.0)); D <- (W D + fbar) / (W + 1); W <- fminf(W + 1,
 *   max_weight).  n_updated counts these voxels; a voxel with N == 0 is neither read nor written.
 *   Touch (hashed, before the accumulate, from the cloud and the pose alone): the block g >> 3 of every in-range sample's voxel is
 *   allocated, whether or not the sdf test skips the sample, under the room rule of icp_tsdf_integrate (table and pool double while a
 *   claim is unplaced).  The set of blocks is exact.
 * Returns ICP_ERR_INVALID_ARG (no volume; which not 0 or 1; a null or non-finite pose; a non-finite sensor_origin; a hashed volume that
 * would have to grow beyond 2^22 blocks) or ICP_ERR_NO_TARGET / ICP_ERR_NO_SOURCE (no such cloud), with a message that names the call and
 * the volume as it was. */
typedef struct icp_tsdf_cloud_info {
    int32_t n_points, n_rays;      /* points of the cloud; those that were usable */
    int32_t n_updated;             /* voxels written */
    int32_t n_blocks;              /* hashed: allocated blocks after the call; dense: 0 */
    int64_t n_samples;             /* in-range samples that reached a voxel */
    int64_t n_outside;             /* samples outside the box (dense) or not storable (hashed; also added to n_out_of_range) */
} icp_tsdf_cloud_info;
#ifdef __cplusplus
static_assert(sizeof(icp_tsdf_cloud_info) == 32, "icp_tsdf_cloud_info");
#endif
int icp_tsdf_integrate_cloud(icp_ctx* ctx, int32_t which, const float pose[16], const float sensor_origin[3], icp_tsdf_cloud_info* info_out);

/* -------- free space carved by the cloud fuses: icp_set_tsdf_carve_options --------
 * An option of the context, off by default.  A scan observes only the band of +- truncation around each return, so something that was
 * scanned and has moved away stays in the model, a single noisy return leaves a speck nothing removes, and the cells at the front edge of
 * the band have unobserved corners.  With distance > 0 every cloud fuse -- icp_tsdf_integrate_cloud and the fuses inside
 * icp_track_scans_sdf -- also observes the voxels IN FRONT of the band, up to `distance` metres before it, wherever storage exists: the
 * existing walk, started earlier.  Carving never allocates, exactly as a depth frame's free-space update never does.  With distance 0 every
 * call launches exactly the kernels it launches without this option.  The options survive new clouds, new volumes and icp_tsdf_reset.
 *
 * Contract (fp32, one rounding per operation, in the order written; tests/tsdf_carve_restatement.py restates it in numpy).  Everything not
 * named here is icp_tsdf_integrate_cloud's, word for word.
 *   J = ceil(min(distance, max_depth) / s), in double; a call whose J exceeds 65536 is refused (ICP_ERR_INVALID_ARG) before any device work.
 *   Samples m = -J .. M, in that order, t_m = fminf((r - truncation) + (float)m s, r + truncation) -- the existing expression.  A sample
 *   with m >= 0 is skipped unless t_m > 0, as without carving; a sample with m < 0 is skipped unless t_m > min_range.  The sample's voxel
 *   and the in-range test are the existing ones.
 *   Repeated voxels, ONE rule for the whole walk: an in-range sample whose voxel equals that of the ray's previous in-range sample is
 *   skipped.  So the ray's first band sample is skipped (and not counted in n_samples) when its voxel was already observed at m = -1; its
 *   observation is the same k either way, because k depends only on ray and voxel.
 *   Observation: an m < 0 sample uses the existing one -- the sdf test, f, k, then S += k, N += 1.  Dense: it applies if the voxel is in
 *   the box.  Hashed: it applies only if the voxel's block is RESIDENT after this call's touch.
 *   Counters: an m < 0 sample without storage, or out of range, does nothing and is counted nowhere.  n_samples and n_outside count
 *   m >= 0 samples only; n_carved counts the applied m < 0 observations.
 *   Touch and fold are unchanged: the hashed touch walks m >= 0 only; n_updated includes the carved voxels.
 * What follows from these rules (the tests lean on it):
 *   (a) Every axis of the voxel sequence along a ray is monotone in m -- each operation between m and g_a is monotone in fp32 -- as the
 *       nearest-voxel sequence of a straight line never returns to a voxel it left (a Voronoi cell is convex).  So a ray observes a voxel
 *       at most once, and skipping samples that have no storage cannot change any result.
 *   (b) A voxel seen only by carve samples whose f = 1 has S = 32768 N, so fbar == 1.0f; from W = 0, D == 1.0f and W == 1, exactly, and
 *       on any voxel W grows by 1.  icp_tsdf_align_cloud's fabsf(F) < 1 drops a point in such a cell; a cell is valid once its corners
 *       are observed.
 *   (c) A voxel that one ray hits and another passes is the integer average of both: the ordinary erosion of carving, not a defect. */
typedef struct icp_tsdf_carve_options {
    float distance;   /* 0 = off (default); > 0 or +inf: metres in front of the band that are carved */
    float min_range;  /* >= 0, finite; carve samples with t <= min_range are skipped (default 0) */
} icp_tsdf_carve_options;
typedef struct icp_tsdf_carve_info {
    int32_t n_steps;          /* J of the last cloud fuse (0: carving was off) */
    int32_t reserved;         /* 0 */
    int64_t n_carved;         /* the carve observations (m < 0) applied by the last cloud fuse */
    int64_t n_carved_total;   /* the same, summed since the options were last set */
} icp_tsdf_carve_info;
#ifdef __cplusplus
static_assert(sizeof(icp_tsdf_carve_options) == 8, "icp_tsdf_carve_options");
static_assert(sizeof(icp_tsdf_carve_info) == 24, "icp_tsdf_carve_info");
#endif
enum { ICP_TSDF_CARVE_MAX_STEPS = 65536 };
int icp_tsdf_carve_options_default(icp_tsdf_carve_options* opt);
/* ICP_OK or ICP_ERR_INVALID_ARG (a negative or NaN distance; a negative or non-finite min_range); needs neither a context nor a device. */
int icp_tsdf_carve_options_check(const icp_tsdf_carve_options* opt);
int icp_set_tsdf_carve_options(icp_ctx* ctx, const icp_tsdf_carve_options* opt);   /* NULL = defaults (off); clears the stats */
int icp_get_tsdf_carve_options(const icp_ctx* ctx, icp_tsdf_carve_options* opt);
int icp_tsdf_carve_stats(const icp_ctx* ctx, icp_tsdf_carve_info* info_out);

/* -------- a laser scan aligned to the TSDF volume itself, and tracked against it --------
 * Direct SDF tracking (icp_tsdf_align_depth above) for a RESIDENT cloud, unorganised, in icp_voxel_map_insert's and
 * icp_tsdf_integrate_cloud's convention (which = 0: the target, 1: the source): every point of the scan, moved into the world by the pose,
 * reads its residual and its normal from the eight voxels around it.  No ray-cast, no target cloud, no index, no search, and no second
 * model beside the volume the scans are fused into.  The volume is whichever the context holds, dense or hashed.  icp_sdf_options is
 * reused: huber, n_iterations, min_valid, stop_rotation and stop_translation mean what they mean for a depth frame; stride must be 1 and is
 * refused otherwise (the order of the resident cloud is internal, so "every s-th point" could not be restated).
 * Unless carving is on (icp_set_tsdf_carve_options) icp_tsdf_integrate_cloud carves no free space, so the field exists only inside the truncation band around the fused surfaces: a point
 * further than the truncation from every surface of the model finds no valid cell and takes no part.  The band is the basin of
 * convergence: only the points that start inside it pull the scan, so the part of the motion between two scans that is normal to the
 * surfaces has to stay inside the truncation for enough of them.
 *
 * Contract (fp32, one rounding per operation, in the order written; everything after the conversion to fp64 is fp64;
 * tests/sdf_cloud_restatement.py restates it in numpy).  P = pose (scan frame -> world, column-major, P_rc = pose[4 c + r]).
 *   Considered: a point (x, y, z) is CONSIDERED iff all three coordinates are finite; n_depth counts the considered points.
 *   Field sample: q_r = (P_r0 x + (P_r1 y + P_r2 z)) + P_r3 -- the depth form's expression with the point's z in place of d.  The cell of
 *   q, its validity, F and the gradient (G_x, G_y, G_z) are icp_tsdf_sample's.
 *   Valid: a point is VALID iff it is considered, its cell is valid and fabsf(F) < 1; n_valid counts the valid points.  There is no
 *   max_depth test: a point has a position, not a range.
 *   Terms, sums, step, stop and failure are the depth form's, word for word: r, g, J and w as there, 28 fp64 sums folded in a fixed order
 *   without floating-point atomics, bitwise reproducible run to run, each within n_valid 2^-52 sum |term| of any other summation order;
 *   the step fails with n_valid < min_valid or a non-finite solution.  An alignment FAILS with no considered point (ICP_ERR_NO_SOURCE) or
 *   a failed step (ICP_ERR_NO_CORRESPONDENCES): it carries the pose it started with.
 *   Order independence: the sums do not depend on the order in which the cloud was uploaded, except by what a summation order may change.
 * Checks come first, without a device and without side effects: ICP_ERR_INVALID_ARG (no volume; which not 0 or 1; a null or non-finite
 * pose; bad options, stride != 1 among them; a null output; n_scans < 1; a null or empty scan) or ICP_ERR_NO_TARGET / ICP_ERR_NO_SOURCE
 * (no such cloud), with a message that names the call.  A refused call leaves the volume bit for bit as it was. */
/* The sums of ONE step at `pose`: sums_out 28 doubles, counts_out {n_depth, n_valid}; of opt only huber matters (stride must be 1). */
int icp_tsdf_cloud_system(icp_ctx* ctx, int32_t which, const float pose[16], const icp_sdf_options* opt, double* sums_out, int32_t* counts_out);
/* Aligns the resident cloud to the volume from pose_inout.  rec_out (optional): the record; trace_out: NULL, or n_iterations records, those
 * past the last step tried zeroed.  Returns the alignment's status; a failed one leaves pose_inout as it was.  One host read. */
int icp_tsdf_align_cloud(icp_ctx* ctx, int32_t which, const icp_sdf_options* opt, float pose_inout[16], icp_sdf_frame* rec_out,
                         icp_sdf_iter* trace_out);
/* Tracking against the model being built: every scan (xyz[k]: n[k] x 3 floats, in its sensor frame) becomes the resident source by
 * icp_track_scans_vmap's upload path.  Scan 0 is fused at pose_inout by icp_tsdf_integrate_cloud's rule (sensor origin: the scan frame's
 * origin); scan k >= 1 is aligned to the volume built so far and, on ICP_OK, fused at the pose found (out[k - 1] its record; out:
 * n_scans - 1 records).  A scan that fails carries the pose, is not fused, records its status, and tracking goes on; the first error in
 * scan order is returned.  infos_out: NULL, or n_scans infos of the fuses, a skipped scan's zeroed.  The host waits once per scan for the
 * record, and as often as icp_tsdf_integrate_cloud does for the fuse.  An error of a fuse (a hashed volume that would have to grow beyond
 * its limit) ends the call. */
int icp_track_scans_sdf(icp_ctx* ctx, const float* const* xyz, const int32_t* n, int32_t n_scans, const icp_sdf_options* opt,
                        float pose_inout[16], icp_sdf_frame* out, icp_tsdf_cloud_info* infos_out);

/* -------- the colours of a laser scan into the coloured TSDF volume --------
 * icp_tsdf_integrate_cloud on a volume WITH colours -- dense with its colour array (icp_tsdf_color_create), or hashed with coloured blocks
 * (icp_tsdf_create_color_hashed) -- and a resident cloud WITH colours (icp_set_target / icp_set_source with rgba): the scan's colours are
 * fused with its geometry, so that everything that reads the colours (icp_tsdf_sample_color, the coloured ray-casts, targets and model
 * loops, icp_tsdf_mesh_color / icp_tsdf_mesh_color_hashed, the coloured evict and insert, the photometric direct tracker) takes a model made
 * from scans as it takes one made from depth frames.
 * Geometry: exactly icp_tsdf_integrate_cloud from the same state under the context's current carve options -- D, W, the blocks, info_out
 * and the carve stats are the same bit for bit.
 * Colour (fp32, one rounding per operation, in the order written; what comes after a cast to double is fp64;
 * tests/tsdf_cloud_color_restatement.py restates it in numpy).  Everything not named here is icp_tsdf_integrate_cloud's, word for word.
 *   Point i's colour is the first three bytes of its rgba, c_0 .. c_2; alpha is not read.
 *   The colour walk of a usable ray is the UNCARVED walk, whatever the carve options are: samples m = 0 .. M with the same t_m, voxel and
 *   in-range test, and the rule about repeated voxels among the ray's own band samples -- a sample whose voxel equals that of the ray's
 *   previous in-range sample with m >= 0 is skipped.  Carve samples (m < 0) never colour.
 *   A band sample colours its voxel iff its observation is not skipped (!(sdf < -truncation)) AND !(sdf > truncation): the band rule of
 *   icp_tsdf_integrate_color.  A band sample's nearest voxel can lie up to about 0.87 voxels nearer the sensor than the sample, so voxels
 *   that are updated and not coloured are common.
 *   The voxel's four integer accumulators take SR += c_0, SG += c_1, SB += c_2, NC += 1.
 *   Fold, for every voxel with NC > 0, with one read of its float4 (C_0, C_1, C_2, Wc): cbar_r = (float)((double)S_r / (double)NC);
 *   C_r <- (Wc C_r + cbar_r) / (Wc + 1.f) per channel; Wc <- fminf(Wc + 1.f, max_weight).  A voxel with NC == 0 has its float4 neither
 *   read nor written.  *n_colored_out (optional) counts the voxels with NC > 0.  The accumulators are all zero outside a call.
 *   On a hashed volume the colour walk visits only voxels whose block this call's touch has made resident; the touch walks the same
 *   m >= 0 samples and is exact.
 *   Limit: the cloud has at most 2^24 points.  By property (a) of the carve contract a ray meets a voxel at most once, so NC <= 2^24 and
 *   every sum is at most 255 2^24 < 2^32: the accumulators are 32-bit, 16 bytes per voxel (8 KiB per pool block of a hashed volume, as much
 *   again as a dense colour array), allocated at the first coloured call; they leave with the volume and are re-made when the storage
 *   they index changes size, as the geometry's accumulators are.
 * What follows from these rules (the tests lean on it): (1) the colours after a call do not depend on the carve options; (2) nor on the
 * order of the points; (3) the coloured voxels are a subset of the updated ones; (4) a voxel coloured by one ray from Wc = 0 holds that
 * point's three bytes exactly, as floats, with Wc == 1.
 * Refusals: icp_tsdf_integrate_cloud's own checks first, in its order; then, all before any device work, a volume without colours
 * (ICP_ERR_INVALID_ARG), a cloud without colours (ICP_ERR_COLOR_MISMATCH), more than 2^24 points (ICP_ERR_INVALID_ARG), each with a message
 * that names the call.  A refused call leaves geometry and colours bit for bit as they were. */
enum { ICP_TSDF_CLOUD_COLOR_MAX_POINTS = 1 << 24 };
int icp_tsdf_integrate_cloud_color(icp_ctx* ctx, int32_t which, const float pose[16], const float sensor_origin[3],
                                   icp_tsdf_cloud_info* info_out, int32_t* n_colored_out);
/* icp_track_scans_sdf with two changes: every scan is uploaded with its colours (rgba[k]: n[k] x 4 bytes) and every fuse is
 * icp_tsdf_integrate_cloud_color's.  The alignment is unchanged and reads geometry only, so poses, records and infos equal
 * icp_track_scans_sdf's on the same scans bit for bit.  n_colored_out: NULL, or n_scans counts, 0 for a skipped scan.  The host waits as
 * often as in icp_track_scans_sdf: n_colored comes back with the counters the fuse reads anyway.  Refused as icp_track_scans_sdf is, then
 * (ICP_ERR_INVALID_ARG, before any scan is uploaded) on a volume without colours, a null rgba or rgba[k], a scan of more than 2^24 points. */
int icp_track_scans_sdf_color(icp_ctx* ctx, const float* const* xyz, const uint8_t* const* rgba, const int32_t* n, int32_t n_scans,
                              const icp_sdf_options* opt, float pose_inout[16], icp_sdf_frame* out, icp_tsdf_cloud_info* infos_out,
                              int32_t* n_colored_out);

/* -------- a coloured laser scan aligned to the coloured TSDF volume with a photometric term --------
 * icp_tsdf_align_cloud with the second row of icp_tsdf_align_depth_color: where the geometry leaves the pose free (a scan of a flat wall or
 * of a floor) the calls above do not move at all; the colours that icp_tsdf_integrate_cloud_color put into the volume pin the scan.  Needs a
 * volume WITH colours, dense (icp_tsdf_color_create) or hashed (icp_tsdf_create_color_hashed), and a resident cloud WITH colours
 * (icp_set_target / icp_set_source with rgba).  tests/sdf_cloud_color_restatement.py restates what follows.
 *
 * Contract (fp32, one rounding per operation, in the order written; everything after a conversion to fp64 is fp64).
 *   Geometric row: considered and valid points, q, the cell, F, G, r, g, J and w are exactly icp_tsdf_cloud_system's.  A point that is not
 *   valid there contributes nothing here either.
 *   Photometric row: icp_tsdf_sdf_system_color's, word for word, with two substitutions -- the moved point q in place of the back-projected
 *   pixel, and the point's own colour, the first three bytes R, G, B of its rgba, in place of the pixel's; the fourth byte is not read.
 *   s_k = (R_k + G_k) + B_k at the eight colour corners of q's cell, S and H as there; a valid point is COLOURED iff all eight corners
 *   have Wc > 0 and S is finite; I_p = (double)(R + G + B) / 765.0; r_c = (double)S / 765.0 - I_p; h = (double)H / (765.0 *
 *   (double)voxel_size); J_c = (q x h, h); w_c = weight^2, with huber > 0 multiplied by (|r_c| <= huber ? 1 : huber / |r_c|).
 *   Sums: 29 doubles in icp_tsdf_sdf_system_color's layout.  A coloured point's term is the geometric term + the photometric term in that
 *   order, a valid point that is not coloured contributes the geometric term alone; entry 28 is (w_c r_c) r_c alone.  Counts: {n_depth,
 *   n_valid, n_color}.  The fold order is fixed, without floating-point atomics: bitwise reproducible run to run, and each sum within
 *   n_valid 2^-52 sum |term| of any other summation order of the same terms, the order of the upload included.
 *   Step, stop, failure, statuses and pose composition: icp_tsdf_align_cloud's, unchanged, on the entries 0 .. 26.
 * Refusals, all before any device work and with a message that names the call: everything icp_tsdf_cloud_system refuses, in its order;
 * then bad colour options (icp_sdf_color_options_check; a weight of zero belongs to the calls above), a volume without colours, a cloud
 * without colours, a null output -- ICP_ERR_INVALID_ARG each. */
/* The sums of ONE joint step at `pose`: sums_out 29 doubles, counts_out {n_depth, n_valid, n_color}; of opt only huber matters. */
int icp_tsdf_cloud_system_color(icp_ctx* ctx, int32_t which, const float pose[16], const icp_sdf_options* opt,
                                const icp_sdf_color_options* copt, double* sums_out, int32_t* counts_out);
/* icp_tsdf_align_cloud with the photometric term: the same outputs in the colour records, the same statuses, one host read. */
int icp_tsdf_align_cloud_color(icp_ctx* ctx, int32_t which, const icp_sdf_options* opt, const icp_sdf_color_options* copt,
                               float pose_inout[16], icp_sdf_color_frame* rec_out, icp_sdf_color_iter* trace_out);
/* icp_track_scans_sdf_color with the photometric alignment: every scan goes up with its colours, scan k >= 1 is aligned by
 * icp_tsdf_align_cloud_color's rule to the volume built so far and, on ICP_OK, fused by icp_tsdf_integrate_cloud_color at the pose found;
 * out: n_scans - 1 colour records.  infos_out, n_colored_out, the carve options, the host waits per scan and the handling of a failed scan
 * are icp_track_scans_sdf_color's.  Refused as that call is (a volume without colours, a null rgba or rgba[k], a scan of more than 2^24
 * points among the reasons), and on bad colour options. */
int icp_track_scans_sdf_photometric(icp_ctx* ctx, const float* const* xyz, const uint8_t* const* rgba, const int32_t* n, int32_t n_scans,
                                    const icp_sdf_options* opt, const icp_sdf_color_options* copt, float pose_inout[16],
                                    icp_sdf_color_frame* out, icp_tsdf_cloud_info* infos_out, int32_t* n_colored_out);

/* -------- a mesh of a chosen resolution (an extension): vertex clustering on the device (Rossignac and Borrel 1993).  DESIGN.md section
 * 6zk. --------
 * The vertices that fall into one cell of a grid become one vertex, a triangle that loses a corner that way is dropped, triangles that
 * become equal are kept once.  One pass, two hash tables and integer sums: the result is a function of the input arrays alone, whatever
 * order the device's threads run in; tests/mesh_cluster_restatement.py restates it in numpy.  Every fp32 operation below is rounded once, in
 * the order written, with no contraction.
 * Cell of a vertex p: per axis r, g = (p_r - o_r) / cell_size and f = floorf(g).  The vertex is INVALID iff a coordinate is not finite or
 *   !(-2^20 <= f < 2^20) on some axis.  Its cell is c_r = (int)f, its offset q_r = (int)((g - f) * 65536.f), in 0 .. 65535 (and 65536 where
 *   g - f rounds up to 1: the cell's far face).
 * Cluster: the valid vertices of one cell; its identity is its FIRST member, the smallest input index.
 * Triangle: INVALID iff an index is >= n_vertices or names an invalid vertex (an index is compared before it is used: nothing is read out of
 *   bounds).  DEGENERATE iff two of its three clusters are equal.  Otherwise it is rotated so that the cluster with the smallest first
 *   member comes first -- orientation kept, never mirrored --, which is its canonical triple.  Triangles with the same canonical triple are
 *   DUPLICATES: the one with the smallest input index survives.  Opposite orientations of the same three clusters are distinct; both stay.
 * Output triangles: the survivors in ascending input index, their corners as written in the input (not rotated), each replaced by the
 *   output index of its cluster.
 * Output vertices: the clusters that a surviving triangle references, in ascending first member; unreferenced clusters are dropped.
 *   n_cells counts all occupied cells, n_vertices the referenced ones.
 * Position of a cluster of n members with the 64-bit integer sums S_r of q_r: Q_r = (2 S_r + n) / (2 n) by integer division,
 *   p'_r = o_r + ((float)c_r + (float)Q_r * 0x1p-16f) * cell_size.
 * Normal (with `normals`): a member whose normal has a non-finite component contributes nothing; otherwise
 *   m_r = (int)rintf(fminf(fmaxf(n_r, -1.f), 1.f) * 32767.f), summed in 64-bit integers to M; N = (float)M,
 *   n' = N / sqrtf(Nx Nx + (Ny Ny + Nz Nz)); a non-finite result is written as (0, 0, 0).
 * Colour (with `colors`, 4 bytes R G B A per vertex): the members with alpha != 0 are the coloured ones, k of them; per channel
 *   (2 Sum + k) / (2 k) by integer division, alpha 255; k = 0: four zero bytes.
 * Consistency: n_triangles + n_degenerate + n_duplicate + n_invalid_triangles == n_triangles_in; two calls give identical arrays.
 * Calling: info_out is required and always written.  All four output arrays NULL: the call only counts.  vertices_out and triangles_out
 *   go together; normals_out needs normals, colors_out needs colors.  vertices_out / normals_out: room for max_vertices * 3 floats,
 *   colors_out for max_vertices * 4 bytes, triangles_out for max_triangles * 3 indices; a count above its capacity:
 *   ICP_ERR_INVALID_ARG, a message with the four numbers, nothing written to the arrays.  cell_size must be finite and > 0, origin finite,
 *   n_vertices and n_triangles in 0 .. 2^27 (ICP_MESH_CLUSTER_MAX).  An empty input or an empty result: ICP_OK with zeros.  Target, source,
 *   volume, params and index stay untouched.  Scratch comes from the context: 16 bytes per slot of the cell table (a power of
 *   two, at least 2 V slots) and 8 per vertex, 4 bytes per slot of the triangle table (at least 2 T) and 20 per triangle, at most 80 per
 *   output vertex for the sums, and the staged input and output.
 * Limits: the representative is the members' mean, so sharp edges are rounded; the result need not be manifold; no error metric is
 *   minimised (quadric error decimation is another algorithm). */
typedef struct icp_mesh_cluster_options { float cell_size; float origin[3]; } icp_mesh_cluster_options;
typedef struct icp_mesh_cluster_info {
    int32_t n_vertices_in, n_triangles_in, n_invalid_vertices, n_invalid_triangles, n_cells, n_vertices, n_triangles, n_degenerate, n_duplicate;
} icp_mesh_cluster_info;
enum { ICP_MESH_CLUSTER_MAX = 1 << 27 };
#ifdef __cplusplus
static_assert(sizeof(icp_mesh_cluster_options) == 16 && sizeof(icp_mesh_cluster_info) == 36, "ABI layout");
#endif
int icp_mesh_cluster(icp_ctx* ctx, int32_t n_vertices, int32_t n_triangles, const float* vertices, const float* normals, const uint8_t* colors,
                     const uint32_t* triangles, const icp_mesh_cluster_options* opt, int32_t max_vertices, int32_t max_triangles,
                     float* vertices_out, float* normals_out, uint8_t* colors_out, uint32_t* triangles_out, icp_mesh_cluster_info* info_out);
/* The model's mesh at a chosen resolution: the extraction of whichever volume the context holds, dense or hashed -- icp_tsdf_mesh,
 * icp_tsdf_mesh_color (with_colors != 0; needs a volume with colours), icp_tsdf_mesh_hashed or icp_tsdf_mesh_color_hashed: the same kernels,
 * the same staged device arrays -- clustered where it lies.  Only the clustered mesh and one small record cross to the host; the
 * full-resolution mesh is never copied.  Contract: the arrays and the info equal, bit for bit and array for array, what icp_mesh_cluster
 * returns for the output of the matching mesh call with normals.  Calling: icp_tsdf_mesh's -- the two count pointers and info_out are required
 * and always written (the counts are the clustered mesh's); all four arrays NULL counts; vertices_out and triangles_out go together;
 * normals_out and colors_out may be NULL, colors_out needs with_colors; capacities and their refusal as above.  No volume, a bad min_weight,
 * bad options, with_colors on a volume without colours, an intermediate mesh of more than 2^27 vertices or triangles:
 * ICP_ERR_INVALID_ARG with a message.  The volume stays as it is. */
int icp_tsdf_mesh_clustered(icp_ctx* ctx, float min_weight, const icp_mesh_cluster_options* opt, int32_t with_colors,
                            int32_t max_vertices, int32_t max_triangles, float* vertices_out, float* normals_out, uint8_t* colors_out,
                            uint32_t* triangles_out, int32_t* n_vertices_out, int32_t* n_triangles_out, icp_mesh_cluster_info* info_out);

/* -------- batches of independent scan pairs: the loop over ETH indices, main.cpp:411-498 / experiment.cpp:319-396 --------
 * The reference aligns the pairs one after the other and carries no state between them, so a batch shards with no
 * data-path exchange: pair p belongs to rank p % n_ranks (icp_pair_owner), and the only collective is ONE gather of the
 * 16-float poses at the end of the batch. */
typedef struct icp_pair {
    const float* src_xyz; const float* src_normals; const uint8_t* src_rgba; int32_t n_src;   /* input.source, borrowed for the call */
    const float* tgt_xyz; const float* tgt_normals; const uint8_t* tgt_rgba; int32_t n_tgt;   /* input.target */
    float initial_pose[16];                                                                  /* estimatedPose on entry (main.cpp:416) */
} icp_pair;

/* Aligns pairs[0..n_pairs) with the contexts ctxs[0..n_ctx) of ONE device: one host thread per context (a context is
 * single-threaded, contexts are independent), each taking the next pair not yet started -- while one pair iterates, the
 * uploads, index builds and iterations of the others overlap on their own HIP streams.  Every context runs with its own
 * icp_params (set them beforehand).  poses_out: n_pairs x 16 floats, column-major, in pair order; status_out (optional):
 * per-pair ICP_OK / error code.  Returns ICP_OK or the first error in pair order. */
int icp_batch_run(icp_ctx* const* ctxs, int32_t n_ctx, const icp_pair* pairs, int32_t n_pairs, float* poses_out, int32_t* status_out);

/* Round-robin ownership of the batch: rank of pair p, and the number of pairs a rank owns. */
int32_t icp_pair_owner(int32_t pair, int32_t n_ranks);
int32_t icp_pairs_of_rank(int32_t n_pairs, int32_t rank, int32_t n_ranks);

/* Pose gather across the GPUs of a node: one RCCL communicator (one rank per process / GPU, xGMI), ONE ncclAllGather of
 * ceil(n_pairs / n_ranks) x 16 floats per rank and batch.  RCCL (librccl.so.1) is loaded on first use, the library has no
 * link-time dependency on it.  The unique id is created on one rank and shipped to the others by the host application
 * (MPI, a file, torch.distributed, ...), exactly like ncclGetUniqueId / ncclCommInitRank. */
typedef struct icp_comm icp_comm;
enum { ICP_COMM_ID_BYTES = 128 };
int icp_comm_unique_id(uint8_t id_out[ICP_COMM_ID_BYTES]);
int icp_comm_create(int device, int32_t n_ranks, int32_t rank, const uint8_t id[ICP_COMM_ID_BYTES], icp_comm** out);
int icp_comm_destroy(icp_comm* comm);
/* local_poses: this rank's poses in the order of its pairs (rank, rank + n_ranks, ...), n_local = icp_pairs_of_rank(...);
 * all_poses_out: n_pairs x 16 floats in pair order, identical on every rank. */
int icp_gather_poses(icp_comm* comm, const float* local_poses, int32_t n_local, int32_t n_pairs, float* all_poses_out);
const char* icp_comm_last_error(void);

/* Library identification: returns e.g. "icp_hip gfx950 <build id>". */
const char* icp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ICP_HIP_H */
