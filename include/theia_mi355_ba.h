/*
 * theia_mi355_ba.h -- C ABI of the MI355X-native bundle-adjustment engine.
 *
 * This is the drop-in boundary for TheiaSfM's full-reconstruction bundle
 * adjustment.  Theia has no FFI / plugin registry for this path: the seam is
 * the C++ API
 *     BundleAdjustReconstruction / BundleAdjustPartialReconstruction
 *         (reference: src/theia/sfm/bundle_adjustment/bundle_adjustment.h:136-155)
 *     class BundleAdjuster { AddView, AddTrack, Optimize }
 *         (reference: src/theia/sfm/bundle_adjustment/bundle_adjuster.h:60-77)
 * whose Optimize() is hard-wired to ceres::Solve
 *         (reference: src/theia/sfm/bundle_adjustment/bundle_adjuster.cc:205).
 * The entry points below are what a maintainer would bind in place of that
 * ceres::Solve call: the host side flattens the Reconstruction into the SoA
 * arrays of tmi_ba_problem, calls tmi_ba_solve(), and copies the in/out arrays
 * back (see INTEGRATION.md for the binding, include/theia/ for the host shim).
 *
 * Plain C, plain pointers and sizes.  No torch / Eigen / Ceres types.
 * All floating point is IEEE fp64, all indices int32 (observation count int64).
 * The library never keeps a caller pointer past the return of a call, never
 * aborts and never throws across this boundary: every entry point returns a
 * tmi_ba_status.
 */
#ifndef THEIA_MI355_BA_H_
#define THEIA_MI355_BA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMI_BA_VERSION_MAJOR 0
#define TMI_BA_VERSION_MINOR 1

/* ---- status codes ------------------------------------------------------ */
typedef enum tmi_ba_status {
  TMI_BA_OK = 0,
  TMI_BA_ERR_INVALID_ARGUMENT = 1, /* null pointer, bad index, bad enum      */
  TMI_BA_ERR_NO_DEVICE = 2,        /* no gfx950 device visible               */
  TMI_BA_ERR_DEVICE = 3,           /* a HIP runtime call failed              */
  TMI_BA_ERR_OUT_OF_MEMORY = 4,
  TMI_BA_ERR_UNSUPPORTED = 5,      /* problem shape the device path lacks    */
  TMI_BA_ERR_EVALUATION_FAILED = 6,/* residual undefined at the start point  */
  TMI_BA_ERR_LINEAR_SOLVER = 7,    /* reduced system could not be solved     */
  TMI_BA_ERR_COLLECTIVE = 8,       /* the all-reduce callback reported error */
  TMI_BA_ERR_CAPACITY = 9,         /* an output array of the caller is too small (tmi_ba_match_features) */
  TMI_BA_ERR_NULL_SPACE_TOO_LARGE = 10, /* tmi_ba_extract_parallel_rigid_subgraph: more than max_null_dimension */
  TMI_BA_ERR_NOT_CONVERGED = 11    /* tmi_ba_extract_parallel_rigid_subgraph: max_iterations reached     */
} tmi_ba_status;

/* ---- enums mirrored from the reference ---------------------------------- */

/* CameraIntrinsicsModelType,
 * reference: src/theia/sfm/camera/camera_intrinsics_model_type.h:45-52.
 * Parameter order inside one intrinsics group:
 *   PINHOLE (7)                  [f, ar, skew, px, py, k1, k2]
 *       reference: pinhole_camera_model.h:86-94
 *   PINHOLE_RADIAL_TANGENTIAL(10)[f, ar, skew, px, py, k1, k2, k3, t1, t2]
 *       reference: pinhole_radial_tangential_camera_model.h:91-102
 *   FISHEYE (9)                  [f, ar, skew, px, py, k1, k2, k3, k4]
 *       reference: fisheye_camera_model.h:67-77
 *   FOV (5)                      [f, ar, px, py, omega]
 *       reference: fov_camera_model.h:69-75
 *   DIVISION_UNDISTORTION (5)    [f, ar, px, py, k]
 *       reference: division_undistortion_camera_model.h:76-82            */
typedef enum tmi_ba_camera_model {
  TMI_BA_PINHOLE = 0,
  TMI_BA_PINHOLE_RADIAL_TANGENTIAL = 1,
  TMI_BA_FISHEYE = 2,
  TMI_BA_FOV = 3,
  TMI_BA_DIVISION_UNDISTORTION = 4
} tmi_ba_camera_model;
#define TMI_BA_MAX_INTRINSICS 10
#define TMI_BA_EXTRINSICS_SIZE 6 /* [C(3), angle_axis(3)], camera.h:195-200 */

/* LossFunctionType,
 * reference: src/theia/sfm/bundle_adjustment/create_loss_function.h:51-58 */
typedef enum tmi_ba_loss {
  TMI_BA_LOSS_TRIVIAL = 0,
  TMI_BA_LOSS_HUBER = 1,
  TMI_BA_LOSS_SOFTLONE = 2,
  TMI_BA_LOSS_CAUCHY = 3,
  TMI_BA_LOSS_ARCTAN = 4,
  TMI_BA_LOSS_TUKEY = 5
} tmi_ba_loss;

/* ceres::LinearSolverType values Theia passes through
 * (reference: bundle_adjustment.h:86; bundle_adjustment.cc:86,100 force
 * DENSE_QR for single view / single track problems).  The device path solves
 * the reduced camera system exactly (blocked dense Cholesky of the explicit
 * Schur complement) for DENSE_QR/DENSE_SCHUR/SPARSE_SCHUR and with
 * preconditioned conjugate gradients for ITERATIVE_SCHUR/CGNR.             */
typedef enum tmi_ba_linear_solver {
  TMI_BA_DENSE_QR = 1,
  TMI_BA_DENSE_SCHUR = 3,
  TMI_BA_SPARSE_SCHUR = 4,
  TMI_BA_ITERATIVE_SCHUR = 5,
  TMI_BA_CGNR = 6
} tmi_ba_linear_solver;

/* ceres::PreconditionerType (bundle_adjustment.h:87).  Substitutions made by the device
 * path, all of them in the PRECONDITIONER only (the reduced system that PCG solves, its
 * stopping rule and therefore the LM step it converges to are the same in every mode; what
 * changes is the number of PCG iterations an LM step takes and the low-order bits of the
 * truncated solve):
 *   SCHUR_JACOBI (Theia's default): the inverse of the block diagonal of the reduced camera
 *     matrix S with ONE block per view = [extrinsics | private intrinsics] merged (up to
 *     16 x 16).  Ceres builds its block diagonal per PARAMETER block, i.e. a 6 x 6
 *     extrinsics block and a separate N x N intrinsics block per view
 *     (schur_jacobi_preconditioner.cc); the merged block keeps the extrinsics-intrinsics
 *     coupling of a view, is a strictly stronger preconditioner and costs the same to apply.
 *   SCHUR_JACOBI_PARAMETER_BLOCKS (extension value, not a ceres enumerator): exactly Ceres's
 *     shape -- the cross terms between a view's extrinsics and intrinsics columns are dropped
 *     before the inversion.  Meant for block-for-block comparisons of PCG trajectories with
 *     real Ceres output (tests/test_ceres_golden.py); slower to converge than the default.
 *   JACOBI maps to SCHUR_JACOBI.
 *   CLUSTER_JACOBI / CLUSTER_TRIDIAGONAL: Ceres clusters the cameras by visibility
 *     (visibility_clustering_type) and inverts the block diagonal of S over the clusters exactly.  Here the
 *     clusters are the intrinsics groups: a cluster = a shared intrinsics block together with the views that share
 *     it, its principal submatrix of S factored densely every LM iteration (6 n_views + <= 10 unknowns) and
 *     applied with two triangular solves per PCG iteration; views of private groups keep their SCHUR_JACOBI block.
 *     Sharing intrinsics puts about three near-degenerate directions per shared block into the block-Jacobi
 *     preconditioned system (principal point against a coherent rotation of the block's views, ...): 45-80 PCG
 *     iterations per LM iteration with SCHUR_JACOBI, 4-5 with the clusters.  Needs the cluster's blocks of S only:
 *     with schur_mode auto (and implicit) the operator PCG applies is the matrix-free one and just the block pairs
 *     INSIDE a cluster are formed for the preconditioner; schur_mode explicit forms all of S.
 *     On problems WITHOUT shared intrinsics blocks the views are clustered by visibility as Ceres'
 *     VisibilityBasedPreconditioner does (visibility_clustering_type below: the Schur-complement graph with
 *     edge weights |tracks seen by both| / sqrt(|tracks of a| |tracks of b|) over the parameter blocks, then
 *     canonical views with size penalty 3 / similarity penalty 0 / at least 3 centres, or single linkage at 0.9;
 *     restated from Ceres 1.14 -- parity unpinned like the rest of the Ceres layer) and every cluster's principal
 *     submatrix of S is inverted exactly; this needs the formed S (schur_mode auto picks it; with schur_mode
 *     implicit, or on several ranks, the solve keeps the SCHUR_JACOBI blocks and says so in
 *     tmi_ba_summary.effective_preconditioner_type).
 *     CLUSTER_TRIDIAGONAL (round 6, cluster_chains.h): Ceres' tridiagonal variant also keeps the blocks between clusters that are neighbours in a degree-2 maximum spanning forest of the cluster graph (vertices: the
 *     clusters above plus every other reduced block as a cluster of its own; edge weight: the number of non-constant
 *     tracks both clusters see; edges taken in decreasing order of (weight, lower end, higher end) unless an end has two
 *     edges already or the ends are connected).  The forest's components are paths; every path is factored exactly as
 *     a block-tridiagonal matrix (a dense factor whose tiles outside the band stay zero: a path is cut where it would
 *     pass TMI_BA_MAX_CLUSTER_DIM unknowns).  Dropping the other blocks can cost positive definiteness: as in Ceres the
 *     off-diagonal cluster-pair cells are then halved and the factorisation repeated once; a second failure fails the
 *     linear solve (an invalid LM step).  Needs the formed S and one rank -- schur_mode auto forms S, schur_mode implicit
 *     and sharded solves keep the SCHUR_JACOBI blocks (effective_preconditioner_type says so).  A handle serves the
 *     preconditioner it was created for (the chains are part of its structure).  Restated from Ceres 1.14
 *     (visibility_based_preconditioner.cc, graph_algorithms.h); parity unpinned like the rest of the Ceres layer.
 *     A cluster launch that cannot become co-resident (device shared with another process) retires
 *     the clusters for that solve: PCG continues with the SCHUR_JACOBI blocks.
 *   Intrinsics shared by several views form their own reduced block in every mode.  */
/* A cluster of CLUSTER_JACOBI is inverted as a dense matrix (n^3 / 3 flops and n^2 / 2 doubles per LM iteration): a
 * cluster with more unknowns than this keeps the SCHUR_JACOBI blocks of its views (Ceres factors its cluster matrices
 * sparsely and has no such limit). */
#define TMI_BA_MAX_CLUSTER_DIM 4096

typedef enum tmi_ba_preconditioner {
  TMI_BA_PRECOND_IDENTITY = 0,
  TMI_BA_PRECOND_JACOBI = 1,
  TMI_BA_PRECOND_SCHUR_JACOBI = 2,
  TMI_BA_PRECOND_CLUSTER_JACOBI = 3,
  TMI_BA_PRECOND_CLUSTER_TRIDIAGONAL = 4,
  TMI_BA_PRECOND_SCHUR_JACOBI_PARAMETER_BLOCKS = 18
} tmi_ba_preconditioner;

/* OptimizeIntrinsicsType bit flags, reference: bundle_adjustment.h:65-76 */
enum {
  TMI_BA_INTRINSICS_NONE = 0x00,
  TMI_BA_INTRINSICS_FOCAL_LENGTH = 0x01,
  TMI_BA_INTRINSICS_ASPECT_RATIO = 0x02,
  TMI_BA_INTRINSICS_SKEW = 0x04,
  TMI_BA_INTRINSICS_PRINCIPAL_POINTS = 0x08,
  TMI_BA_INTRINSICS_RADIAL_DISTORTION = 0x10,
  TMI_BA_INTRINSICS_TANGENTIAL_DISTORTION = 0x20,
  TMI_BA_INTRINSICS_ALL = 0x3f
};

/* camera_flags bits: which half of the 6 extrinsics is held constant
 * (reference: bundle_adjuster.cc:304-334; both bits = SetCameraExtrinsicsConstant,
 * which is also what AddTrack does to cameras that were not added through
 * AddView, bundle_adjuster.cc:156-168).                                     */
enum {
  TMI_BA_CAMERA_POSITION_CONSTANT = 0x1,
  TMI_BA_CAMERA_ORIENTATION_CONSTANT = 0x2
};

/* ---- the flattened problem ---------------------------------------------- */
/* Caller-owned structure-of-arrays view of the residual set
 *   {(view, track): view estimated, track estimated, view observes track}
 * that BundleAdjuster::AddView/AddTrack build (bundle_adjuster.cc:102-180).
 * Arrays marked in/out are overwritten with the optimised values when the
 * solve produced a usable solution (Ceres semantics: CONVERGENCE or
 * NO_CONVERGENCE, bundle_adjuster.cc:218) and left untouched otherwise.     */
typedef struct tmi_ba_problem {
  /* cameras (one per optimised or anchoring view) */
  int32_t num_cameras;
  double* extrinsics;            /* in/out [6*num_cameras]                   */
  const int32_t* camera_group;   /* [num_cameras] intrinsics group index     */
  const uint8_t* camera_flags;   /* [num_cameras] TMI_BA_CAMERA_* bits       */

  /* shared intrinsics groups (reference: reconstruction.h:93-106; one Ceres
   * parameter block per group because Camera holds a shared_ptr, camera.h:247) */
  int32_t num_groups;
  const int32_t* group_model;    /* [num_groups] tmi_ba_camera_model         */
  const int32_t* group_offset;   /* [num_groups+1] offsets into intrinsics   */
  double* intrinsics;            /* in/out [group_offset[num_groups]]        */
  const uint8_t* intrinsics_constant; /* same length; 1 = held constant
                                    (GetSubsetFromOptimizeIntrinsicsType and
                                    the whole-block rule bundle_adjuster.cc:242-287) */

  /* tracks: homogeneous 3-D points (reference: track.h:66-67) */
  int32_t num_points;
  double* points;                /* in/out [4*num_points]                    */
  const uint8_t* point_constant; /* [num_points] 1 = SetTrackConstant        */

  /* observations: Feature = pixel (x, y) (reference: feature.h) */
  int64_t num_observations;
  const int32_t* obs_camera;     /* [num_observations]                       */
  const int32_t* obs_point;      /* [num_observations]                       */
  const double* obs_xy;          /* [2*num_observations]                     */
} tmi_ba_problem;

/* ---- options: BundleAdjustmentOptions field for field -------------------- */
/* reference: src/theia/sfm/bundle_adjustment/bundle_adjustment.h:78-122.
 * intrinsics_to_optimize / constant_camera_* live in the flattened problem
 * (intrinsics_constant, camera_flags); tmi_ba_intrinsics_constant_mask()
 * below converts the bitmask.                                               */
typedef struct tmi_ba_options {
  int32_t loss_function_type;        /* tmi_ba_loss, default TRIVIAL         */
  double robust_loss_width;          /* 2.0                                   */
  int32_t linear_solver_type;        /* tmi_ba_linear_solver, SPARSE_SCHUR    */
  int32_t preconditioner_type;       /* tmi_ba_preconditioner, SCHUR_JACOBI   */
  int32_t verbose;                   /* 0                                     */
  int32_t num_threads;               /* accepted, unused by the device path   */
  int32_t max_num_iterations;        /* 100                                   */
  double max_solver_time_in_seconds; /* 3600                                  */
  int32_t use_inner_iterations;      /* 1 (reference default, bundle_adjustment.h:112): after
                                        every trust-region step one coordinate-descent sweep
                                        over extrinsics blocks, intrinsics blocks, points
                                        (Ceres inner iterations in the reversed solver
                                        ordering, bundle_adjuster.cc:193-200), until their relative gain
                                        drops below 1e-3; evaluated in fp64 whatever
                                        residual_precision says                  */
  double function_tolerance;         /* 1e-6                                  */
  double gradient_tolerance;         /* 1e-10                                 */
  double parameter_tolerance;        /* 1e-8                                  */
  double max_trust_region_radius;    /* 1e12                                  */

  /* Ceres defaults Theia does not override; exposed so the
   * benchmark and the tests can pin them.                                    */
  double initial_trust_region_radius; /* 1e4                                  */
  double min_trust_region_radius;     /* 1e-32                                */
  double min_relative_decrease;       /* 1e-3                                 */
  double min_lm_diagonal;             /* 1e-6                                 */
  double max_lm_diagonal;             /* 1e32                                 */
  double eta;                         /* 0.1  (PCG forcing, q-tolerance)      */
  int32_t max_linear_solver_iterations; /* 500                                */
  int32_t min_linear_solver_iterations; /* 0                                  */
  int32_t max_num_consecutive_invalid_steps; /* 5                             */
  int32_t jacobi_scaling;             /* 1                                    */

  /* extensions of the device path */
  int32_t point_dof;       /* 4 = reference-exact homogeneous points (no
                              parameterization, bundle_adjuster.cc:379-385);
                              3 = hold w fixed (the north-star 2x3 blocks)   */
  int32_t device;          /* HIP device ordinal; -1 = current device        */
  int32_t profile_kernels; /* 1 = bracket every kernel class with HIP events
                              and report per-class times in the summary      */
  int32_t residual_precision; /* 64 = fp64 throughout (reference precision).
                              32 = residuals and Jacobian blocks evaluated in fp32
                              (camera translation still removed in fp64), loss
                              correction and all accumulation (J^T J, gradients,
                              cost) in fp64 -- BASELINE config 5.  Fixed at
                              tmi_ba_solver_create.                                */
  int32_t schur_mode;      /* ITERATIVE_SCHUR only.  1 = explicit: form the block
                              sparse reduced camera matrix S (Schur complement) and
                              run PCG on it; with several GPUs S is all-reduced once
                              per LM iteration.  2 = implicit: S is never formed, every
                              PCG product walks the observations (Ceres'
                              ImplicitSchurComplement), with several GPUs one small
                              all-reduce (the reduced vector) per PCG iteration.
                              0 = auto: implicit on several GPUs; on one GPU both
                              operators are kept resident and every LM iteration takes
                              the cheaper one for the PCG length it expects (forming S
                              pays off after a few products; same result to round-off). */
  int32_t visibility_clustering_type;
                           /* CLUSTER_JACOBI / CLUSTER_TRIDIAGONAL on a problem WITHOUT shared
                              intrinsics blocks: how the views are clustered (ceres::
                              VisibilityClusteringType, bundle_adjustment.h:88-89; Theia's default is
                              CANONICAL_VIEWS).  0 = CANONICAL_VIEWS, 1 = SINGLE_LINKAGE.          */
  double* iteration_trace; /* optional (NULL = none): HOST buffer of iteration_trace_capacity rows of
                              TMI_BA_TRACE_STRIDE doubles, one row per trust-region iteration (the first
                              summary.num_iterations rows, fewer if the buffer is shorter):
                              [0] iteration (1-based), [1] cost at the iteration's linearisation point,
                              [2] trust-region radius the step was computed with, [3] outcome (1 accepted,
                              0 rejected, -1 invalid step, 2 parameter tolerance reached, 3 function
                              tolerance reached -- 2 and 3 drop the candidate), [4] candidate cost (NaN for an
                              invalid step), [5] model cost change, [6] linear-solver (PCG) iterations of this
                              iteration, [7] step norm.  What ceres::Solver::Summary::iterations holds; the
                              reference reads none of it (bundle_adjuster.cc:203-218) -- it exists so that
                              tests can hold the trust-region trajectory against an independent model
                              (tests/trajectory_model.py).  On a sharded solve every rank writes the same rows. */
  int32_t iteration_trace_capacity;
} tmi_ba_options;
#define TMI_BA_TRACE_STRIDE 8

/* ---- summary: BundleAdjustmentSummary + device-path extras --------------- */
/* reference: bundle_adjustment.h:125-133 */
#define TMI_BA_NUM_KERNEL_CLASSES 12
typedef struct tmi_ba_summary {
  int32_t success;               /* IsSolutionUsable()                       */
  double initial_cost;           /* 1/2 sum rho(|r|^2)                       */
  double final_cost;
  double setup_time_in_seconds;  /* flatten-side preprocessing + upload      */
  double solve_time_in_seconds;  /* the LM loop, device-resident inputs      */

  int32_t status;                /* tmi_ba_status                            */
  int32_t termination;           /* 0 convergence, 1 no convergence (limits),
                                    2 failure                                */
  int32_t num_iterations;        /* LM iterations run (accepted + rejected)  */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int64_t num_linear_solver_iterations; /* PCG iterations over the solve     */
  double final_rmse;             /* sqrt(sum |r|^2 / num_obs), un-robustified */
  double initial_rmse;
  int32_t num_reduced_blocks;    /* camera blocks of the reduced system      */
  int32_t reduced_block_dim;     /* D (uniform, zero padded)                 */
  int64_t num_schur_blocks;      /* structurally non-zero D x D blocks of S,
                                    upper triangle incl. diagonal            */
  int64_t num_schur_pairs;       /* observation pairs feeding off-diagonal S */
  int32_t num_inner_iteration_steps; /* LM iterations that ran an inner-iteration sweep */
  int32_t num_matrix_free_iterations; /* LM iterations whose PCG ran on the matrix-free operator
                                         (all of them with schur_mode 2; some with auto on one rank) */
  /* per kernel class (index = tmi_ba_kernel_class): launches and total
   * device time from HIP events; filled when options.profile_kernels != 0   */
  int64_t kernel_launches[TMI_BA_NUM_KERNEL_CLASSES];
  double kernel_seconds[TMI_BA_NUM_KERNEL_CLASSES];
  char message[192];
  /* the preconditioner PCG actually ran with in the last LM iteration (tmi_ba_preconditioner_type; 0 for the exact
   * solvers): differs from options.preconditioner_type where the header above says a request is served by another
   * one -- CLUSTER_JACOBI without usable clusters (several ranks, schur_mode implicit without shared blocks, a
   * cluster launch that could not become co-resident, clusters that do not fit) keeps its SCHUR_JACOBI blocks,
   * JACOBI runs as SCHUR_JACOBI.  A caller can tell which trajectory it got. */
  int32_t effective_preconditioner_type;
} tmi_ba_summary;

typedef enum tmi_ba_kernel_class {
  TMI_BA_K_LINEARIZE = 0,      /* residuals + Jacobian blocks per observation */
  TMI_BA_K_POINT_ELIMINATE = 1,/* per-track V, g_p, (V+D)^-1, Y = W L^-T     */
  TMI_BA_K_CAMERA_DIAG = 2,    /* per-camera U, g~, diagonal S block          */
  TMI_BA_K_SCHUR_OFFDIAG = 3,  /* off-diagonal S blocks from pair lists       */
  TMI_BA_K_PRECONDITIONER = 4, /* invert diagonal blocks                      */
  TMI_BA_K_SPMV = 5,           /* q = S p (PCG)                               */
  TMI_BA_K_PCG_VECTOR = 6,     /* PCG dots / axpys / preconditioner apply     */
  TMI_BA_K_CHOLESKY = 7,       /* dense reduced-system factor + solve         */
  TMI_BA_K_BACK_SUBSTITUTE = 8,/* delta_p, model cost change                  */
  TMI_BA_K_UPDATE_COST = 9,    /* x+ = x + delta, trial cost                  */
  TMI_BA_K_REDUCE = 10,        /* small reductions / bookkeeping              */
  TMI_BA_K_ALLREDUCE = 11      /* time spent inside the all-reduce callback   */
} tmi_ba_kernel_class;

/* ---- multi-GPU hook ------------------------------------------------------- */
/* When the tracks are sharded over several processes (one per GPU) each rank
 * builds the reduced camera system from its own tracks; the engine then calls
 * this hook once per LM iteration on the concatenated device buffer
 *   [S blocks | U diagonal | reduced gradient | cost terms]
 * and once (a few doubles) for the trial cost.  The hook must sum `count`
 * doubles in place across ranks (RCCL all-reduce over xGMI in practice) on
 * `stream` or synchronise it itself.  Return 0 on success.                  */
typedef int (*tmi_ba_allreduce_fn)(void* device_buffer, int64_t count,
                                   void* hip_stream, void* user);

/* ---- entry points --------------------------------------------------------- */
typedef struct tmi_ba_solver tmi_ba_solver; /* opaque, device-resident problem */

/* Library / device discovery. */
int32_t tmi_ba_version(void);           /* major*1000 + minor                 */
int32_t tmi_ba_device_count(void);      /* gfx950 devices visible, <0 = error */
const char* tmi_ba_status_string(int32_t status);
/* Human-readable detail of the last failed call on the calling thread. */
const char* tmi_ba_last_error(void);

/* Fill `opts` with the reference defaults (bundle_adjustment.h:78-122 plus
 * the Ceres defaults of SURVEY App. B). */
void tmi_ba_options_init(tmi_ba_options* opts);

/* Number of intrinsic parameters of a camera model (kIntrinsicsSize), or -1. */
int32_t tmi_ba_intrinsics_size(int32_t camera_model);

/* GetSubsetFromOptimizeIntrinsicsType for one model
 * (reference: pinhole_camera_model.cc:132-162 and the four siblings):
 * writes 1 into mask[i] for every parameter held constant under the
 * OptimizeIntrinsicsType bitmask.  mask has tmi_ba_intrinsics_size() entries. */
int32_t tmi_ba_intrinsics_constant_mask(int32_t camera_model,
                                        int32_t intrinsics_to_optimize,
                                        uint8_t* mask);

/* One-shot: upload, solve, download.  The replacement for ceres::Solve at
 * bundle_adjuster.cc:205.  Re-entrant; serialises per device.               */
int32_t tmi_ba_solve(tmi_ba_problem* problem, const tmi_ba_options* options,
                     tmi_ba_summary* summary);

/* Resident form (used by the benchmark so the timed region starts with the
 * inputs already in HBM, and by pipelines that run BA -> filter -> BA):
 *   create   : validate, build the static structure (track-major and
 *              camera-major orders, Schur block structure, pair lists),
 *              upload.  `rank`/`world` select the contiguous shard of tracks
 *              this process owns (0/1 for single GPU).
 *   solve    : run LM on the resident parameters (may be called repeatedly).  The options of a solve need not
 *              be the ones of create: schur_mode, residual_precision, device and (outside the cluster
 *              preconditioners) visibility_clustering_type are fixed at create and ignored here -- the solve
 *              gives the bits of create's values -- while a point_dof that differs is TMI_BA_ERR_INVALID_ARGUMENT.
 *   reset    : restore the parameters uploaded at create time (or by the last set_parameters).
 *   set_parameters : new values of extrinsics / intrinsics / points for the SAME residual set and
 *              constancy flags (the caller moved cameras or re-triangulated tracks between two
 *              BAs): uploads them and makes them what `reset` restores; the structure, the
 *              layouts and every buffer stay resident.
 *   download : copy the current parameters into the caller's in/out arrays.  */
int32_t tmi_ba_solver_create(const tmi_ba_problem* problem,
                             const tmi_ba_options* options, int32_t rank,
                             int32_t world, tmi_ba_solver** out);
int32_t tmi_ba_solver_set_allreduce(tmi_ba_solver* s, tmi_ba_allreduce_fn fn,
                                    void* user);
/* Native RCCL transport (optional, instead of the hook).  The engine resolves
 * ncclGetUniqueId / ncclCommInitRank / ncclAllReduce at run time from the librccl
 * already loaded in the process (PyTorch's) or from /opt/rocm, and issues
 * ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, comm, engine stream) itself:
 *   rank 0 : tmi_ba_rccl_unique_id(id)  -> ship the 128 bytes to every rank
 *   all    : tmi_ba_solver_init_rccl(solver, id)   (rank / world from create)
 * A hook set with tmi_ba_solver_set_allreduce is ignored once RCCL is initialised;
 * tmi_ba_solver_init_rccl(solver, NULL) destroys the communicator again (fall back to the hook). */
int32_t tmi_ba_rccl_unique_id(uint8_t id[128]);
int32_t tmi_ba_solver_init_rccl(tmi_ba_solver* s, const uint8_t id[128]);
/* Test aid: sums the solver's 8-double scalar buffer through the configured
 * transport (even for world = 1) after filling it with `value`; returns the
 * first element in *out. */
int32_t tmi_ba_solver_debug_allreduce(tmi_ba_solver* s, double value, double* out);
int32_t tmi_ba_solver_solve(tmi_ba_solver* s, const tmi_ba_options* options,
                            tmi_ba_summary* summary);
int32_t tmi_ba_solver_reset(tmi_ba_solver* s);
int32_t tmi_ba_solver_set_parameters(tmi_ba_solver* s, const tmi_ba_problem* problem);
int32_t tmi_ba_solver_download(tmi_ba_solver* s, tmi_ba_problem* problem);
/* The HIP stream the engine launches on (so callers can record their own
 * events on it). */
void* tmi_ba_solver_stream(tmi_ba_solver* s);
void tmi_ba_solver_destroy(tmi_ba_solver* s);

/* Per-observation evaluation on the device, exposed for parity tests:
 * residuals [2*N], the reduced camera Jacobian blocks [2*D*N] (row major
 * 2 x D, columns = free extrinsics then free PRIVATE intrinsics of the observing
 * camera), the Jacobian w.r.t. the free intrinsics the camera SHARES with other
 * views [2*D*N] (zero when it shares none) and point Jacobian blocks
 * [2*point_dof*N], in the caller's observation order, without loss correction
 * or Jacobi scaling.  valid[i] = 0 where the reference functor returns false
 * (reprojection_error.h:75-77).  Any output pointer may be NULL.            */
int32_t tmi_ba_solver_evaluate(tmi_ba_solver* s, double* residuals,
                               double* jac_camera, double* jac_shared,
                               double* jac_point, uint8_t* valid,
                               int32_t* block_dim);

/* ---- steps either side of the full adjustment ----------------------- */

/* Post-BA outlier filter: theia::SetOutlierTracksToUnestimated
 * (src/theia/sfm/set_outlier_tracks_to_unestimated.cc:62-133; callers
 * global_reconstruction_estimator.cc:259-263, incremental_reconstruction_estimator.cc:525,592).
 * Every camera and track of the flattened problem counts as estimated.  Per track:
 *   flag 1  a projection lies behind its camera (Camera::ProjectPoint depth < 0, :101-105) or
 *           the mean squared reprojection error exceeds max_inlier_reprojection_error^2 (:110-115)
 *   flag 2  no pair of viewing rays subtends min_triangulation_angle_degrees
 *           (SufficientTriangulationAngle, triangulation.cc:236-250; :120-125)
 *   flag 0  the track stays estimated.
 * The caller applies the flags (Track::SetEstimated(false)); the return value of the
 * reference is num_bad_reprojections + num_insufficient_viewing_angles. */
typedef struct tmi_ba_filter_summary {
  int64_t num_estimated_tracks;
  int64_t num_bad_reprojections;
  int64_t num_insufficient_viewing_angles;
  double seconds;        /* wall time of the call */
  double kernel_seconds; /* the device kernel alone (HIP events) */
} tmi_ba_filter_summary;

/* On the parameters resident in `solver` (e.g. right after tmi_ba_solver_solve: nothing is
 * uploaded).  track_flag / track_mean_sq_error are indexed by the caller's track index,
 * [num_points]; entries of tracks owned by other ranks are left untouched and the counts
 * cover this rank's tracks.  Either output may be NULL. */
int32_t tmi_ba_solver_filter_outlier_tracks(tmi_ba_solver* solver,
                                            double max_inlier_reprojection_error,
                                            double min_triangulation_angle_degrees,
                                            uint8_t* track_flag, double* track_mean_sq_error,
                                            tmi_ba_filter_summary* summary);

/* One-shot form: uploads the problem, filters, frees everything. device < 0 = current. */
int32_t tmi_ba_filter_outlier_tracks(const tmi_ba_problem* problem, int32_t device,
                                     double max_inlier_reprojection_error,
                                     double min_triangulation_angle_degrees, uint8_t* track_flag,
                                     double* track_mean_sq_error, tmi_ba_filter_summary* summary);

/* Batched theia::BundleAdjustTrack (bundle_adjustment.cc:96-107, called once per track from
 * estimate_track.cc:238-246): every non-constant track of the problem is adjusted on its own
 * with all cameras and intrinsics held constant -- one independent trust-region problem per
 * GPU thread, same Levenberg-Marquardt semantics and options as tmi_ba_solve (the linear
 * solve is the track's own point_dof x point_dof system; linear_solver_type is irrelevant,
 * max_solver_time_in_seconds is not enforced).
 * track_termination[num_points]: 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE, 3 residual
 * evaluation failed at the start point, -1 not adjusted (constant or unobserved track).
 * BundleAdjustmentSummary::success of the per-track call == (termination is 0 or 1); points
 * are updated exactly in that case.  All per-track outputs may be NULL. */
typedef struct tmi_ba_track_batch_summary {
  int64_t num_tracks;       /* tracks adjusted */
  int64_t num_success;
  int64_t total_iterations; /* sum of LM iterations over the tracks */
  double seconds;
  double kernel_seconds;
} tmi_ba_track_batch_summary;

int32_t tmi_ba_solver_adjust_tracks(tmi_ba_solver* solver, const tmi_ba_options* options,
                                    int8_t* track_termination, int32_t* track_iterations,
                                    double* track_initial_cost, double* track_final_cost,
                                    tmi_ba_track_batch_summary* summary);

/* One-shot form; problem->points is updated in place. */
int32_t tmi_ba_adjust_tracks(tmi_ba_problem* problem, const tmi_ba_options* options,
                             int8_t* track_termination, int32_t* track_iterations,
                             double* track_initial_cost, double* track_final_cost,
                             tmi_ba_track_batch_summary* summary);

/* Batched theia::BundleAdjustView (bundle_adjustment.cc:83-93; called once per newly localised view from
 * localize_view_to_reconstruction.cc:248-252, for a whole list of views per round by
 * incremental_reconstruction_estimator.cc:219-233).  The result equals calling the per-view path
 * (tmi_ba_solve on the view's one-view problem, linear_solver_type DENSE_QR, no inner iterations) once for
 * every selected view in ascending camera index order, each call starting from the parameters the previous
 * calls left:
 *   - view_mask[num_cameras] selects the views (NULL = all).  A selected view's free parameters are its
 *     extrinsics minus the halves camera_flags fix, and the free entries (intrinsics_constant == 0) of its
 *     intrinsics group; its residuals are its own observations under the options' loss.  Every point is
 *     constant and never written; views that are not selected neither move nor contribute residuals, even
 *     when they share the selected view's group (what BundleAdjuster::AddView alone builds,
 *     bundle_adjuster.cc:102-135).
 *   - Two selected views of a group with free entries run one after the other (a CHAIN): the later one starts
 *     from the intrinsics the earlier one produced.  Views that share no free group are independent and run
 *     concurrently, one 256-thread workgroup per chain, all chains in one launch, longest first.
 *   - The trust-region loop is tmi_ba_solve's (Jacobi scaling, LM radius rules, function / gradient /
 *     parameter tolerances, max_num_iterations, max_num_consecutive_invalid_steps); the linear step is the
 *     exact solve of the view's damped D x D normal equations (D <= 16).  max_solver_time_in_seconds is not
 *     enforced; evaluation is fp64 whatever residual_precision says; linear_solver_type, preconditioner_type,
 *     use_inner_iterations and point_dof are irrelevant.
 * view_termination[num_cameras]: 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE, 3 residual evaluation failed at
 * the start point (reprojection_error.h:75-77; tmi_ba_solve's TMI_BA_ERR_EVALUATION_FAILED: both costs 0),
 * -1 not adjusted (not selected, no observations, or nothing free).  Extrinsics and group intrinsics are
 * written back exactly when the code is 0 or 1 (IsSolutionUsable).  All per-view outputs may be NULL. */
typedef struct tmi_ba_view_batch_summary {
  int64_t num_views;        /* views adjusted (termination >= 0) */
  int64_t num_success;      /* termination 0 or 1 */
  int64_t total_iterations; /* sum of LM iterations over the views */
  int64_t num_chains;       /* workgroups of the launch (chains of views run in sequence) */
  double seconds;           /* wall time of the call */
  double kernel_seconds;    /* the device kernel alone (HIP events) */
} tmi_ba_view_batch_summary;

/* One-shot form: uploads the cameras, the groups, the points and the observations of the views to adjust (no Schur
 * structure), adjusts, updates problem->extrinsics / intrinsics in place.  The device is options->device
 * (-1 = current). */
int32_t tmi_ba_adjust_views(tmi_ba_problem* problem, const tmi_ba_options* options, const uint8_t* view_mask,
                            int8_t* view_termination, int32_t* view_iterations, double* view_initial_cost,
                            double* view_final_cost, tmi_ba_view_batch_summary* summary);

/* Resident form: on the parameters already in `solver` (e.g. right after tmi_ba_solver_solve or
 * tmi_ba_solver_set_parameters); nothing is uploaded.  The first call builds a view-major index of the
 * handle's observations on the device (radix sort of (view, slot) keys) and keeps it in the handle; it does
 * not depend on the reduced-block layout, so views without a reduced block (constant views) can be selected.
 * The camera-derived caches of the handle are invalidated, so a later tmi_ba_solver_solve / download sees the
 * new cameras.  TMI_BA_ERR_INVALID_ARGUMENT on a sharded handle (world > 1). */
int32_t tmi_ba_solver_adjust_views(tmi_ba_solver* solver, const tmi_ba_options* options, const uint8_t* view_mask,
                                   int8_t* view_termination, int32_t* view_iterations, double* view_initial_cost,
                                   double* view_final_cost, tmi_ba_view_batch_summary* summary);

/* Batched theia::TrackEstimator (src/theia/sfm/estimate_track.cc:205-264; called from
 * global_reconstruction_estimator.cc:438-452 and incremental_reconstruction_estimator.cc): every selected track is
 * (re)estimated from scratch from its observations, every camera of the problem counting as an estimated view and
 * held constant.  The input point of a selected track is ignored.  Per track:
 *   1. fewer than 2 observations                                         -> status 1
 *   2. rays: Camera::PixelToUnitDepthRay(pixel).normalized() (camera.cc:215-223): R^T times the model's
 *      PixelToCameraCoordinates (the iterative UndistortPoint of PINHOLE, RADIAL_TANGENTIAL and FISHEYE: at most
 *      100 steps, stop at |delta| < 1e-10 per coordinate; FOV and DIVISION closed form), R from
 *      ceres::AngleAxisToRotationMatrix
 *   3. no pair of rays with dot < cos(min_triangulation_angle_degrees) (SufficientTriangulationAngle,
 *      triangulation.cc:236-250)                                         -> status 1
 *   4. TriangulateMidpoint (triangulation.cc:130-157): A = sum (I - d d^T), b = sum (I - d d^T) [C; 1] over the
 *      4 x 4 homogeneous form, Eigen's LLT (a pivot <= 0 fails)          -> status 2 on failure
 *   5. bundle_adjustment != 0: BundleAdjustTrack with ba_options (bundle_adjustment.cc:96-107; the trust-region
 *      loop of tmi_ba_adjust_tracks); a termination other than CONVERGENCE / NO_CONVERGENCE -> status 3, the point
 *      keeps the triangulated value
 *   6. AcceptableReprojectionError (estimate_track.cc:90-115): any Camera::ProjectPoint depth < 0, or a mean
 *      squared reprojection error not below max_acceptable_reprojection_error_pixels^2 -> status 4
 *   otherwise status 0: the track is estimated (the caller calls Track::SetEstimated(true)).
 * track_status[num_points] (int8): -1 not attempted (not selected, or a constant point), 0..4 as above.  Points
 * are written for statuses 0, 3 and 4 (where the reference writes Track::MutablePoint) and left untouched for
 * -1, 1 and 2.  track_mask[num_points]: 1 = estimate (NULL = every track).  track_status may be NULL.
 * ba_options->point_dof chooses the point parameterisation of step 5 and of the handle. */
typedef struct tmi_ba_track_estimator_options {
  double max_acceptable_reprojection_error_pixels; /* 5.0 (estimate_track.h:63-64) */
  double min_triangulation_angle_degrees;          /* 3.0 (estimate_track.h:66-69) */
  int32_t bundle_adjustment;                       /* 1   (estimate_track.h:71-73) */
} tmi_ba_track_estimator_options;

void tmi_ba_track_estimator_options_init(tmi_ba_track_estimator_options* options);

typedef struct tmi_ba_track_estimate_summary {
  int64_t num_attempts;             /* tracks with a status >= 0 */
  int64_t num_estimated;            /* status 0 */
  int64_t num_bad_angle;            /* status 1 (the reference's num_bad_angles_) */
  int64_t num_failed_triangulation; /* status 2 */
  int64_t num_failed_ba;            /* status 3 */
  int64_t num_bad_reprojection;     /* status 4 */
  double seconds;                   /* wall time of the call */
  double kernel_seconds;            /* the device kernels alone (HIP events) */
} tmi_ba_track_estimate_summary;

/* One-shot form: uploads the problem (no Schur structure), estimates, updates problem->points in place.  The
 * device is ba_options->device (-1 = current). */
int32_t tmi_ba_estimate_tracks(tmi_ba_problem* problem, const tmi_ba_track_estimator_options* estimator_options,
                               const tmi_ba_options* ba_options, const uint8_t* track_mask, int8_t* track_status,
                               tmi_ba_track_estimate_summary* summary);

/* Resident form: the selected tracks of the handle from the handle's cameras; nothing is uploaded but the mask.
 * The cameras do not move, so the handle's camera-derived caches stay valid, and which tracks a later
 * tmi_ba_solver_solve includes does not change.  A selected track without observations gets status 1.
 * TMI_BA_ERR_INVALID_ARGUMENT on a sharded handle (world > 1) or when ba_options->point_dof differs from the
 * handle's. */
int32_t tmi_ba_solver_estimate_tracks(tmi_ba_solver* solver, const tmi_ba_track_estimator_options* estimator_options,
                                      const tmi_ba_options* ba_options, const uint8_t* track_mask,
                                      int8_t* track_status, tmi_ba_track_estimate_summary* summary);

/* Pre-BA track sub-sampling: theia::SelectGoodTracksForBundleAdjustment
 * (src/theia/sfm/select_good_tracks_for_bundle_adjustment.cc:251-327; callers
 * global_reconstruction_estimator.cc:475-486, incremental_reconstruction_estimator.cc:497-515).
 * Track statistics (:81-110: observation count truncated at long_track_length_threshold, mean
 * squared reprojection error over all observations) are computed on the device; the
 * selection logic runs on the host:
 *   1. per view, the features are binned into image_grid_cell_size_pixels cells and the
 *      track with the minimum (truncated length, mean error) of every occupied cell is
 *      selected (:150-196 with the comparator at :65-69);
 *   2. per view, if fewer than min_num_optimized_tracks_per_view of its tracks are selected,
 *      the not yet selected ones with the smallest track index are added (:201-249 ranks
 *      std::pair<TrackId, statistics> with the default operator<).
 * The reference iterates unordered containers; the engine fixes what that leaves open: views
 * in ascending index order, grid-cell ties to the smaller track index.
 * view_mask[num_cameras] (NULL = every view): the views whose features take part in steps 1
 * and 2 -- the reference's overload with an explicit view set (:280-327); the statistics of a
 * track always cover all of its observations (:81-110).
 * selected[num_points] (required): 1 = optimise this track.  stats_len / stats_err
 * [num_points] may be NULL.  Needs an unsharded handle (world == 1). */
typedef struct tmi_ba_select_summary {
  int64_t num_tracks;
  int64_t num_selected;
  int64_t num_selected_grid; /* selected by the grid step alone */
  double seconds;
  double kernel_seconds;     /* the statistics kernel (HIP events) */
} tmi_ba_select_summary;

int32_t tmi_ba_solver_select_good_tracks(tmi_ba_solver* solver, int32_t long_track_length_threshold,
                                         int32_t image_grid_cell_size_pixels,
                                         int32_t min_num_optimized_tracks_per_view,
                                         const uint8_t* view_mask, uint8_t* selected,
                                         int32_t* stats_len, double* stats_err,
                                         tmi_ba_select_summary* summary);

int32_t tmi_ba_select_good_tracks(const tmi_ba_problem* problem, int32_t device,
                                  int32_t long_track_length_threshold,
                                  int32_t image_grid_cell_size_pixels,
                                  int32_t min_num_optimized_tracks_per_view,
                                  const uint8_t* view_mask, uint8_t* selected,
                                  int32_t* stats_len, double* stats_err,
                                  tmi_ba_select_summary* summary);

/* Batched theia::BundleAdjustTwoViews (src/theia/sfm/bundle_adjustment/bundle_adjust_two_views.cc:
 * 113-191; called once per verified view pair from two_view_match_geometric_verification.cc:285):
 * every pair is an independent small bundle adjustment -- camera 1 extrinsics constant, camera 2
 * extrinsics free, each camera's intrinsics constant or free in the focal length only (:66-98),
 * one homogeneous point per correspondence seen by both cameras, no loss, DENSE_SCHUR, at most
 * max_num_iterations (the reference: 200) iterations, otherwise Ceres' default solver options
 * (SetSolverOptions :58-68).  One wavefront per pair runs the pair's whole trust-region solve.
 * Arrays are caller-owned; extrinsics2, intrinsics1/2 (focal length) and points are updated in place
 * for the pairs whose termination is 0 or 1 (Ceres' IsSolutionUsable).
 *   point_dof: 4 = the reference (no point parameterization); 3 holds the homogeneous w fixed.
 *   pair_termination / pair_iterations / pair_initial_cost / pair_final_cost [num_pairs] may be NULL;
 *   termination: 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE, 3 residual evaluation failed at the
 *   start point, -1 pair without correspondences. */
typedef struct tmi_ba_two_view_batch {
  int32_t num_pairs;
  const double* extrinsics1;            /* [6 * num_pairs] held constant                       */
  double* extrinsics2;                  /* [6 * num_pairs] in/out                              */
  const int32_t* model1;                /* [num_pairs] tmi_ba_camera_model                     */
  const int32_t* model2;
  double* intrinsics1;                  /* [10 * num_pairs] model order, zero padded; in/out   */
  double* intrinsics2;
  const uint8_t* constant_intrinsics1;  /* [num_pairs] TwoViewBundleAdjustmentOptions flags;   */
  const uint8_t* constant_intrinsics2;  /*   NULL = constant (the reference default)           */
  const int64_t* correspondence_ptr;    /* [num_pairs + 1] ranges into the arrays below        */
  const double* features1;              /* [2 * N] pixel in image 1                            */
  const double* features2;              /* [2 * N] pixel in image 2                            */
  double* points;                       /* [4 * N] homogeneous points, in/out                  */
} tmi_ba_two_view_batch;

int32_t tmi_ba_adjust_two_views(tmi_ba_two_view_batch* batch, int32_t point_dof,
                                int32_t max_num_iterations, int32_t device,
                                int8_t* pair_termination, int32_t* pair_iterations,
                                double* pair_initial_cost, double* pair_final_cost,
                                tmi_ba_track_batch_summary* summary);

/* ---- batched two-view verification BA: triangulate, adjust, filter ------------------------
 * reference: TwoViewMatchGeometricVerification::BundleAdjustRelativePose
 * (src/theia/sfm/two_view_match_geometric_verification.cc:256-324), the one caller of BundleAdjustTwoViews, with the
 * two tests VerifyMatches puts around it (:171-176, :181).  The input per pair is what that function has: the two
 * cameras (SetupCameras :56-68), the two constant-intrinsics flags (:276-279) and the pair's correspondences in
 * pixels; batch->points is an OUTPUT only (its input is ignored).  For a pair with n correspondences:
 *   1. n <= min_num_inlier_matches: BundleAdjustRelativePose is not entered (:171-176) and :181 cannot hold
 *                                                                        -> pair status 1, nothing written
 *   2. TriangulatePoints (:185-254), per correspondence in input order:
 *      rays Camera::PixelToUnitDepthRay(feature).normalized() of both cameras (:209-211; as step 2 of
 *      tmi_ba_estimate_tracks);
 *      SufficientTriangulationAngle (:212-216; dot < cos(min_triangulation_angle_degrees)) fails
 *                                                                        -> correspondence status 1
 *      TriangulateMidpoint over the origins {C1, C2} (:218-222; the 4 x 4 homogeneous form and Eigen's LLT rule of
 *      step 4 of tmi_ba_estimate_tracks) fails                           -> correspondence status 2
 *      AcceptableReprojectionError (:72-83) in camera 1, then camera 2, against
 *      triangulation_max_reprojection_error (:226-238): a Camera::ProjectPoint depth < 0, or a squared error not
 *      strictly below the squared threshold                              -> correspondence status 3
 *      the survivors are compacted in their original order (:240-241, :253)
 *   3. fewer than min_num_inlier_matches survivors (:268; `<`)           -> pair status 2, no adjustment
 *   4. BundleAdjustTwoViews on the survivors (:272-289): tmi_ba_adjust_two_views' solve, bit for bit; a termination
 *      other than CONVERGENCE / NO_CONVERGENCE (:291-293)                -> pair status 3, cameras untouched
 *   5. the filter after the adjustment (:295-314): the same two-camera test against final_max_reprojection_error on
 *      the adjusted cameras and points                                   -> correspondence status 4 where it fails
 *   6. more than min_num_inlier_matches correspondences left (:181; `>`) -> pair status 0, otherwise 4.  For both,
 *      extrinsics2 and the two focal lengths are updated in place: the reference updates the TwoViewInfo (:316-321)
 *      before VerifyMatches applies that last test.
 * correspondence_status[N] (int8): -1 not attempted (pair status 1), 0 kept, 1..4 as above.  A 0 means "verified" only
 * in a pair of status 0 or 4; in a pair of status 2 or 3 it marks the survivors of the triangulation.
 * points are written for the correspondences of status 0 and 4: adjusted in pairs of status 0 / 4, the triangulated
 * value in pairs of status 2 / 3.  pair_num_verified[num_pairs]: the pair's correspondences at status 0.
 * pair_termination / pair_iterations / pair_initial_cost / pair_final_cost: those of tmi_ba_adjust_two_views
 * (termination -1 where no adjustment ran).  Every per-pair and per-correspondence output may be NULL.
 * bundle_adjustment == 0 stops after step 3: pair status 0 or 2, the triangulated points written at their original
 * indices.  That mode is NOT a path of the reference (which calls this function only to adjust): it is an extension
 * for staging the steps and for tests.
 * One wavefront per pair in three launches (triangulate, solve, accept); a pair's result does not depend on the rest
 * of the batch.  The RANSAC of EstimateTwoViewInfo (:128-134) that precedes this step is provided for both branches:
 * tmi_ba_estimate_uncalibrated_relative_poses (eight-point) and tmi_ba_estimate_calibrated_relative_poses (five-point,
 * inlier-count scoring; MLESAC scoring is not provided) below.  Out of scope: guided matching (:157-168)
 * and the homography inlier count (:124). */
typedef struct tmi_ba_two_view_verification_options {
  int32_t min_num_inlier_matches;               /* 30   (two_view_match_geometric_verification.h:59-92) */
  double triangulation_max_reprojection_error;  /* 15.0 */
  double min_triangulation_angle_degrees;       /* 4.0  */
  double final_max_reprojection_error;          /* 5.0  */
  int32_t bundle_adjustment;                    /* 1    */
} tmi_ba_two_view_verification_options;

void tmi_ba_two_view_verification_options_init(tmi_ba_two_view_verification_options* options);

typedef struct tmi_ba_two_view_verification_summary {
  int64_t num_pairs;                         /* pairs of the batch */
  int64_t num_pairs_verified;                /* pair status 0 */
  int64_t num_pairs_too_few_matches;         /* pair status 1 */
  int64_t num_pairs_too_few_triangulated;    /* pair status 2 */
  int64_t num_pairs_failed_ba;               /* pair status 3 */
  int64_t num_pairs_too_few_verified;        /* pair status 4 */
  int64_t num_correspondences;               /* correspondences with a status >= 0 */
  int64_t num_verified;                      /* correspondence status 0 */
  int64_t num_bad_triangulation_angles;      /* 1 (the reference's VLOG counters, :198-200) */
  int64_t num_failed_triangulations;         /* 2 */
  int64_t num_bad_reprojection_errors;       /* 3 */
  int64_t num_bad_final_reprojection_errors; /* 4 (:312-313) */
  int64_t total_iterations;                  /* sum of LM iterations over the adjusted pairs */
  double seconds;                            /* wall time of the call */
  double kernel_seconds;                     /* all launches of the call (HIP events) */
  double triangulate_kernel_seconds;         /* its split: two_view_triangulate_kernel */
  double solve_kernel_seconds;               /*            two_view_lm_kernel */
  double accept_kernel_seconds;              /*            two_view_accept_kernel: kernel_seconds minus the two
                                              *            above, not an event pair of its own */
} tmi_ba_two_view_verification_summary;

int32_t tmi_ba_verify_two_views(tmi_ba_two_view_batch* batch, const tmi_ba_two_view_verification_options* options,
                                int32_t point_dof, int32_t max_num_iterations, int32_t device,
                                int8_t* correspondence_status, int8_t* pair_status, int32_t* pair_num_verified,
                                int8_t* pair_termination, int32_t* pair_iterations, double* pair_initial_cost,
                                double* pair_final_cost, tmi_ba_two_view_verification_summary* summary);

/* ---- batched BundleAdjustTwoViewsAngular --------------------------------------------------
 * reference: bundle_adjust_two_views.cc:193-240 -- the relative pose of a view pair from
 * its correspondences alone: parameters TwoViewInfo::rotation_2 (angle-axis, 3) and
 * TwoViewInfo::position_2 (3, kept on the unit sphere by
 * AutoDiffLocalParameterization<UnitNormThreeVectorParameterization, 3, 3>,
 * unit_norm_three_vector_parameterization.h:45-63), one AngularEpipolarError residual per
 * correspondence (angular_epipolar_error.h:47-89; features in normalised image coordinates), no
 * loss, DENSE_SCHUR with the ordering left to Ceres, at most 200 iterations, Ceres' default
 * tolerances.  One wavefront per pair on the device.  Termination codes as for
 * tmi_ba_adjust_two_views; rotation2 / position2 are written back for usable solutions. */
typedef struct tmi_ba_two_view_angular_batch {
  int32_t num_pairs;
  double* rotation2;                    /* [3 * num_pairs] in/out                              */
  double* position2;                    /* [3 * num_pairs] in/out, unit norm                   */
  const int64_t* correspondence_ptr;    /* [num_pairs + 1] ranges into the arrays below        */
  const double* features1;              /* [2 * N] normalised image coordinates in view 1      */
  const double* features2;              /* [2 * N] ... in view 2                               */
} tmi_ba_two_view_angular_batch;

int32_t tmi_ba_adjust_two_views_angular(tmi_ba_two_view_angular_batch* batch, int32_t max_num_iterations,
                                        int32_t device, int8_t* pair_termination, int32_t* pair_iterations,
                                        double* pair_initial_cost, double* pair_final_cost,
                                        tmi_ba_track_batch_summary* summary);

/* ---- batched OptimizeRelativePositionWithKnownRotation -------------------------------------
 * reference: optimize_relative_position_with_known_rotation.cc:53-197, called once per view-graph edge
 * by RefineRelativeTranslationsWithKnownRotations (reconstruction_estimator_utils.cc:244-269) -- the
 * unit direction of camera 2's position in camera 1's frame from the pair's correspondences and the
 * two known world-to-camera rotations: constraint columns c_i = R1 (R2^T [f2_i; 1] x R1^T [f1_i; 1])
 * (:53-79), iteratively reweighted least squares on t^T c_i = 0 (:128-184; at most 100 iterations,
 * stopping once the change max(|cost - new cost|, 1 - t^T t) stayed <= 1e-5 for 10 iterations in a
 * row, weights clamped at 1e-7 -- the reference's constants, not options), then t -> -t unless more
 * than n / 2 correspondences triangulate in front of both cameras (:189-194, triangulation.cc:216-232).
 * The position is an output only (the reference overwrites its argument before reading it).
 * Views and pairs: an orientation per view and an edge list, as the caller of the global pipeline has
 * them.  With view_model / view_intrinsics the features are pixels and the device normalises them
 * (PixelToNormalizedCoordinates(...).hnormalized(), reconstruction_estimator_utils.cc:84-88).
 * One wavefront per pair on the device; a pair's result does not depend on the rest of the batch.
 *   pair_status: 0 converged, 1 stopped at 100 iterations (position2 written for both, as the
 *   reference returns true for both), 2 non-finite input (position2 untouched), -1 pair without
 *   correspondences (untouched).  pair_cost: the final sum of |t^T c_i|.  pair_num_in_front: the
 *   correspondences in front of both cameras for the returned sign.  Where neither sign has a
 *   majority the returned sign is implementation-defined (in the reference: by its SVD).
 *   All per-pair outputs may be NULL.  summary: num_tracks = pairs with correspondences,
 *   num_success = pairs with status 0 or 1, total_iterations = IRLS iterations over the pairs. */
typedef struct tmi_ba_relative_position_batch {
  int32_t num_views;
  const double*  view_rotation;     /* [3 * num_views] angle-axis, world to camera                      */
  const int32_t* view_model;        /* [num_views] tmi_ba_camera_model; NULL = features are normalised   */
  const double*  view_intrinsics;   /* [10 * num_views] model order, zero padded; NULL with view_model   */
  int32_t num_pairs;
  const int32_t* pair_view1;        /* [num_pairs] */
  const int32_t* pair_view2;
  const int64_t* correspondence_ptr;/* [num_pairs + 1] */
  const double*  features1;         /* [2 * N] normalised coordinates, or pixels when view_model != NULL */
  const double*  features2;
  double*        position2;         /* [3 * num_pairs] OUT (untouched for status -1 / 2)                */
} tmi_ba_relative_position_batch;

int32_t tmi_ba_optimize_relative_positions(tmi_ba_relative_position_batch* batch, int32_t device,
                                           int8_t* pair_status, int32_t* pair_iterations,
                                           double* pair_cost, int32_t* pair_num_in_front,
                                           tmi_ba_track_batch_summary* summary);

/* ---- the view-pair filters of the global pipeline's edge stage -------------------------------
 * The view table and edge list of tmi_ba_relative_position_batch with a TwoViewInfo per edge.  No view pairs itself
 * and no unordered pair appears twice (the reference's edges are keys of a map). */
typedef struct tmi_ba_view_pair_batch {
  int32_t num_views;
  const double*  view_rotation;   /* [3 * num_views] angle-axis, world to camera; for the translation filter
                                     NULL = pair_position2 is already in the global frame                    */
  int32_t num_pairs;
  const int32_t* pair_view1;      /* [num_pairs] */
  const int32_t* pair_view2;
  const double*  pair_rotation2;  /* [3 * num_pairs] TwoViewInfo::rotation_2 (orientation filter only)       */
  const double*  pair_position2;  /* [3 * num_pairs] TwoViewInfo::position_2 (translation filter only)       */
} tmi_ba_view_pair_batch;

/* FilterViewPairsFromRelativeTranslation, the 1DSfM filter of Wilson and Snavely
 * (filter_view_pairs_from_relative_translation.cc; called at global_reconstruction_estimator.cc:392).
 *   1. :68-85    t_e = AngleAxisRotatePoint(-view_rotation[view1], position_2), Ceres' formula with its small-angle
 *                branch; skipped when view_rotation is NULL.
 *   2. :180-195  the mean over the edges and the sum of squared deviations / (E - 1), by a reduction of fixed shape.
 *                E < 2 leaves the variance undefined: TMI_BA_ERR_INVALID_ARGUMENT unless the axes are given.
 *   3. :216-221  axes_given != 0: the caller's axes as they are (unit norm is the caller's business).  Otherwise
 *                num_iterations axes are drawn on the host from `seed`: three normal deviates with mean mean[k] and
 *                standard deviation variance[k] -- the reference passes the variance where RandGaussian takes a
 *                standard deviation, and so does this call -- then divided by their norm (left alone if that is 0).
 *                The generator is the engine's own and deterministic in `seed`: state = seed, every 64-bit word is
 *                one splitmix64 step (Steele, Lea and Flood 2014), u = ((word >> 11) + 0.5) 2^-53, and deviates come
 *                in Box-Muller pairs sqrt(-2 ln u1) (cos, sin)(2 pi u2), cosine first; component k of axis i is
 *                deviate 3 i + k (the unused half of the last pair is dropped).  It does not equal
 *                std::normal_distribution.  The axes used are written to `axes` when that is not NULL.
 *   4.           per iteration and edge p = t.x a.x + t.y a.y + t.z a.z, left to right, never contracted into FMA.
 *   5. :114-163  OrderTranslationsFromProjections on the directed graph: p > 0 is view1 -> view2, otherwise
 *                view2 -> view1 (a zero projection is an edge of weight 0 in the reversed direction and counts as an
 *                incoming node); weight |p|; a view's initial incoming / outgoing weight is the sequential sum over
 *                its edges in ascending edge index.  Then one step per view with an edge (:90-110): a remaining
 *                view without remaining incoming nodes if there is one -- THE ONE WITH THE SMALLEST INDEX, where the
 *                reference takes the first its hash map yields -- else the remaining view with the largest
 *                (outgoing_weight + 1.0) / (incoming_weight + 1.0), TIES TO THE SMALLEST INDEX.  The chosen view
 *                gets the step's number as its order; every remaining neighbour loses the edge's weight from the
 *                matching sum, and an incoming node where the edge pointed at it.  Views without edges: order -1.
 *   6. :233-251  d = order[view2] - order[view1]; (d < 0 && p > 0) || (d > 0 && p < 0) contributes |p|.
 *                pair_bad_weight is the sum of the contributions IN ASCENDING ITERATION ORDER from zero (the
 *                reference adds in thread-completion order).
 *   7. :294-304  pair_removed = pair_bad_weight > translation_projection_tolerance * num_iterations.
 * One workgroup per iteration on the device, all iterations in one launch.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: a null batch, options or summary, a missing array,
 * a view index out of range, view1 == view2, a repeated unordered pair, num_iterations < 1, a non-finite rotation,
 * position or given axis, axes_given without axes.  num_pairs == 0: OK, nothing written.
 * Every output may be NULL: pair_removed [num_pairs], pair_bad_weight [num_pairs], rotated_translation
 * [3 * num_pairs], iteration_order [num_iterations * num_views]. */
typedef struct tmi_ba_translation_filter_options {
  int32_t  num_iterations;                    /* 48 (the reference recommends more than 40)  */
  double   translation_projection_tolerance;  /* 0.08, tau of the paper                      */
  uint64_t seed;                              /* 0                                           */
} tmi_ba_translation_filter_options;
void tmi_ba_translation_filter_options_init(tmi_ba_translation_filter_options* options);

typedef struct tmi_ba_view_pair_filter_summary {
  int32_t num_pairs;
  int32_t num_pairs_removed;
  int32_t num_iterations;      /* 0 for the orientation filter                          */
  int32_t num_views_ordered;   /* views with at least one edge; 0 for the orientation filter */
  double  seconds;
  double  kernel_seconds;
} tmi_ba_view_pair_filter_summary;

int32_t tmi_ba_filter_view_pairs_from_relative_translation(const tmi_ba_view_pair_batch* batch,
                                                           const tmi_ba_translation_filter_options* options,
                                                           double* axes, int32_t axes_given, int32_t device,
                                                           uint8_t* pair_removed, double* pair_bad_weight,
                                                           double* rotated_translation, int32_t* iteration_order,
                                                           tmi_ba_view_pair_filter_summary* summary);

/* FilterViewPairsFromOrientation (filter_view_pairs_from_orientation.cc:55-122; called at
 * global_reconstruction_estimator.cc:360).  Per edge loop = R(-rotation_2) (R(orientation2) R(-orientation1))
 * (:60-63), removed when the squared rotation angle of loop exceeds the squared threshold in radians (:64-67,
 * :80-84).  The reference takes the angle as the norm of RotationMatrixToAngleAxis(loop); only that norm is used, and
 * it is computed here from the matrix as atan2(|skew part| / 2, (trace - 1) / 2), in [0, pi].  pair_angle: radians.
 * A view without an orientation (:94-103) has no counterpart in a dense table: the host shim removes such edges.
 * One thread per edge, one launch.  TMI_BA_ERR_INVALID_ARGUMENT as above, and for a negative or NaN threshold (the
 * reference CHECK_GEs it).  pair_removed and pair_angle [num_pairs] may be NULL. */
int32_t tmi_ba_filter_view_pairs_from_orientation(const tmi_ba_view_pair_batch* batch,
                                                  double max_relative_rotation_difference_degrees, int32_t device,
                                                  uint8_t* pair_removed, double* pair_angle,
                                                  tmi_ba_view_pair_filter_summary* summary);

/* ---- RobustRotationEstimator: global orientations from relative rotations ---------------------
 * reference: robust_rotation_estimator.cc:66-282 (GlobalRotationEstimatorType::ROBUST_L1L2, the default; Chatterjee and
 * Govindu, ICCV 2013) with math/l1_solver.h:120-178 and math/rotation.cc:122-132.  The orientations every view-pair
 * call above takes come out of this one.
 * The batch is an edge list on a dense view table.  UNLIKE tmi_ba_view_pair_batch the same unordered pair may occur
 * more than once and in either direction (AddRelativeRotationConstraint, robust_rotation_estimator.h:93-103). */
typedef struct tmi_ba_relative_rotation_batch {
  int32_t num_views;
  int32_t num_pairs;
  const int32_t* pair_view1;     /* [num_pairs] */
  const int32_t* pair_view2;
  const double*  pair_rotation;  /* [3 * num_pairs] angle-axis R_12 = R_2 R_1^T (TwoViewInfo::rotation_2) */
} tmi_ba_relative_rotation_batch;

/* RobustRotationEstimator::Options (robust_rotation_estimator.h:63-82) with the reference's defaults. */
typedef struct tmi_ba_robust_rotation_options {
  int32_t max_num_l1_iterations;            /* 5; 0 skips the L1 phase       */
  double  l1_step_convergence_threshold;    /* 1e-3                          */
  int32_t max_num_irls_iterations;          /* 100; 0 skips the IRLS phase   */
  double  irls_step_convergence_threshold;  /* 1e-3                          */
  double  irls_loss_parameter_sigma;        /* 5 degrees in radians          */
} tmi_ba_robust_rotation_options;
void tmi_ba_robust_rotation_options_init(tmi_ba_robust_rotation_options* options);

typedef struct tmi_ba_robust_rotation_summary {
  int32_t num_views;
  int32_t num_pairs;
  int32_t num_l1_iterations;      /* outer L1 iterations run                                   */
  int32_t num_admm_iterations;    /* ADMM iterations over all of them                          */
  int32_t num_irls_iterations;
  int32_t l1_converged;           /* the L1 phase stopped at its step threshold                */
  int32_t irls_converged;         /* the IRLS phase stopped at its step threshold              */
  int32_t num_factorizations;     /* dense Cholesky factorisations of order num_views - 1      */
  double  seconds;
  double  kernel_seconds;         /* device time; the sum of the three below                   */
  double  factor_seconds;         /* Laplacian assembly + factorisation                        */
  double  substitution_seconds;   /* forward / backward substitution                           */
  double  graph_seconds;          /* the per-edge and per-view kernels and their reductions    */
} tmi_ba_robust_rotation_summary;

/* EstimateRotations on the device.  view_rotation [3 * num_views] holds the initial orientations (angle-axis, world to
 * camera) and receives the result; view `fixed_view` keeps its value (the reference holds fixed whichever view its hash
 * map yields first).
 *   1. :101-147  A has a -I3 block at view1 and a +I3 block at view2 of every edge, without the fixed view's columns.
 *                Free view v has column v - (v > fixed_view); n = num_views - 1.  The IRLS weights are one scalar per
 *                edge, so A^T W A = L_w (x) I3 with L_w the weighted graph Laplacian without the fixed view's row and
 *                column: every solve is ONE dense symmetric positive definite system of order n with three right-hand
 *                sides, factored by the blocked Cholesky of the exact camera solve.  Parallel edges add into L_w in
 *                ascending edge index.
 *   2. :256-272  r_e = MultiplyRotations(-o[view2], MultiplyRotations(rotation_e, o[view1])), MultiplyRotations
 *                (math/rotation.cc:122-132) being Ceres' AngleAxisToRotationMatrix on both, the matrix product and Ceres'
 *                RotationMatrixToAngleAxis (through the quaternion, as Ceres 1.x).
 *   3. :149-171  L1 phase: up to max_num_l1_iterations outer iterations of (L1Solver::Solve on b = r, step 4, step 2),
 *                stopping at average step <= l1_step_convergence_threshold.  The ADMM budget is 5 in the first outer
 *                iteration and doubles with every further one.  L_1 (unit weights) is factored once for the phase.
 *      l1_solver.h:120-178, per Solve: z = u = 0; per iteration x = (A^T A)^-1 A^T (b + z - u); Ax_hat = alpha A x +
 *                (1 - alpha)(z + b); z_old = z; z = Shrinkage(Ax_hat - b + u, 1 / rho); u += Ax_hat - z - b; stop when
 *                |A x - z - b| < sqrt(3 E) 1e-4 + 1e-2 max(|A x|, |z|, |b|) and |rho A^T (z - z_old)| <
 *                sqrt(3 n) 1e-4 + 1e-2 |rho A^T u|.  rho = alpha = 1, the tolerances 1e-4 and 1e-2: the reference's
 *                constants, not options.
 *   4. :240-252, :274-282  o[v] = MultiplyRotations(o[v], step[v]) for the free views; the average step is the mean of
 *                |step[v]| over them.
 *   5. :173-236  IRLS phase: up to max_num_irls_iterations iterations of w_e = sigma / (|r_e|^2 + sigma^2)^2, one
 *                factorisation of L_w, step = L_w^-1 A^T W r, step 4, step 2, stopping at average step <
 *                irls_step_convergence_threshold (strictly).
 *   6.           Fixed orders: edges in the caller's order; every per-view sum over the view's edges from zero in
 *                ascending edge index; every sum over the edges or the views by a reduction of fixed shape (a binary
 *                tree over blocks of 256, the block sums strided over 256 accumulators in ascending order, the same
 *                tree again).  The result is the same bits from call to call.
 * The loops run on the host; every kernel is a plain grid launch.  A non-positive pivot: TMI_BA_ERR_LINEAR_SOLVER.
 * n is capped at 11000 (the dense matrix, 8 n^2 bytes, stays under 1 GB; the environment variable
 * TMI_BA_ROTATION_MAX_ORDER lowers the cap, a diagnostic knob): TMI_BA_ERR_UNSUPPORTED above it, before anything is
 * allocated.  A sparse factorisation for larger graphs is not provided.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: a null batch, options, view_rotation or summary, a
 * missing array, num_pairs == 0 (the reference CHECK_GTs it), a view index out of range, view1 == view2, fixed_view out
 * of range, a non-finite orientation or relative rotation, a threshold or sigma that is not positive and finite, a
 * negative iteration count, and a view that the edges do not connect to fixed_view (L_w would be singular; the
 * reference's callers pass the largest connected component).
 * On every failure view_rotation and the optional outputs are left as they were.  Optional outputs (each may be NULL):
 * pair_residual [3 * num_pairs] the final r; l1_admm_iterations / l1_average_step [max_num_l1_iterations] per outer L1
 * iteration run; irls_average_step / irls_squared_residual [max_num_irls_iterations] the average step and |r|^2 after
 * every IRLS iteration run. */
int32_t tmi_ba_estimate_global_rotations_robust(const tmi_ba_relative_rotation_batch* batch,
                                                const tmi_ba_robust_rotation_options* options, int32_t fixed_view,
                                                int32_t device, double* view_rotation, double* pair_residual,
                                                int32_t* l1_admm_iterations, double* l1_average_step,
                                                double* irls_average_step, double* irls_squared_residual,
                                                tmi_ba_robust_rotation_summary* summary);

/* ---- LeastUnsquaredDeviationPositionEstimator: camera positions from orientations and directions ----
 * reference: least_unsquared_deviation_position_estimator.cc:75-212 (GlobalPositionEstimatorType::
 * LEAST_UNSQUARED_DEVIATION; Ozyesil and Singer, CVPR 2015) with math/constrained_l1_solver.cc:49-187; called at
 * global_reconstruction_estimator.cc EstimatePosition, after the rotation estimator and the view-pair filters above.
 * The estimator builds ConstrainedL1Solver with DEFAULT options (its own Options are only CHECKed), so the defaults
 * below are constrained_l1_solver.h:64-74. */
typedef struct tmi_ba_lud_position_options {
  int32_t max_num_iterations;   /* 1000 */
  double  rho;                  /* 10   */
  double  alpha;                /* 1.2  */
  double  absolute_tolerance;   /* 1e-4 */
  double  relative_tolerance;   /* 1e-2 */
} tmi_ba_lud_position_options;
void tmi_ba_lud_position_options_init(tmi_ba_lud_position_options* options);

typedef struct tmi_ba_lud_position_summary {
  int32_t num_views;
  int32_t num_pairs;
  int32_t num_admm_iterations;
  int32_t converged;              /* both stopping tests held before max_num_iterations ran out    */
  int32_t num_factorizations;     /* dense Cholesky factorisations of order 3 (num_views - 1): 1    */
  double  seconds;
  double  kernel_seconds;         /* device time; the sum of the three below                        */
  double  factor_seconds;         /* directions, assembly of S and its factorisation                */
  double  substitution_seconds;   /* forward / backward substitution                                */
  double  graph_seconds;          /* the per-edge and per-view kernels and their reductions         */
} tmi_ba_lud_position_summary;

/* EstimatePositions on the device.  The batch is tmi_ba_view_pair_batch: view_rotation (or NULL: pair_position2 is
 * already in the global frame), pair_view1 / pair_view2 and pair_position2; pair_rotation2 is not read.
 * view_position [3 * num_views] receives the positions; view `fixed_view` is at 0 (the reference holds fixed whichever
 * view its hash map yields first).
 *   1. :56-63, :177-181  t_e = R(view_rotation[view1])^T position_2 with R Ceres' AngleAxisToRotationMatrix (not
 *                AngleAxisRotatePoint): (R^T p)[k] = (R(0, k) p0 + R(1, k) p1) + R(2, k) p2.
 *   2. :154-212, :90-97  The unknowns are the positions of the n = num_views - 1 free views -- free view v has columns
 *                3 (v - (v > fixed_view)) + c -- then one scale s_e per edge, column 3 n + e.  Rows 3 e + c:
 *                p[view2] - p[view1] - s_e t_e; rows 3 E + e: s_e.  b = [0 (3 E); 1 (E)].
 *   3.           With d_e = |t_e|^2 + 1 = (t0 t0 + t1 t1) + t2 t2 + 1 and W_e = I3 - t_e t_e^T / d_e, eliminating the
 *                scales from A^T A leaves S of order 3 n: the diagonal block of view v is the sum of W_e over its edges in
 *                ascending edge index, block (view1, view2) of an edge is -W_e, the fixed view's rows and columns are
 *                absent.  S is positive definite exactly when every view reaches fixed_view.  It is factored ONCE by the
 *                blocked Cholesky of the exact camera solve.  With q = A^T (b + z - u) = [q_p; q_s] the solve is
 *                p = S^-1 (q_p with t_e (q_s[e] / d_e) subtracted at view1 and added at view2) and
 *                s_e = (q_s[e] + t_e . (p[view2] - p[view1])) / d_e.  The reference factors the whole sparse matrix of
 *                order 3 n + E with Eigen / CHOLMOD; the two differ only in rounding.
 *   4. constrained_l1_solver.cc:112-170  z = u = 0; per iteration x = (A^T A)^-1 A^T (b + z - u) (step 3);
 *                Ax_hat = alpha A x + (1 - alpha)(z + b); z_old = z; z = ModifiedShrinkage(Ax_hat - b + u, 1 / rho), the
 *                first 3 E rows by the shrinkage of l1_solver.h, the last E rows by max(., 0); u += Ax_hat - z - b; stop
 *                when, strictly, |A x - z - b| < sqrt(4 E) absolute_tolerance + relative_tolerance max(|A x|, |z|, |b|)
 *                and |rho A^T (z - z_old)| < sqrt(3 n + E) absolute_tolerance + relative_tolerance |rho A^T u|.  The
 *                result is the x of the last iteration run.
 *   5.           Fixed orders: edges in the caller's order; every per-view sum over the view's edges from zero in
 *                ascending edge index; every norm by a reduction of fixed shape (a binary tree over blocks of 256, the
 *                block sums strided over 256 accumulators in ascending order, the same tree again); for the two norms
 *                of A^T products the edges' block sums (the scale entries) come before the views' (the position entries)
 *                in that second stage.  No expression is contracted into FMA.  The result is the same bits from call to
 *                call.
 * The loop runs on the host; every kernel is a plain grid launch.  A non-positive pivot: TMI_BA_ERR_LINEAR_SOLVER.
 * 3 n is capped at 11000, i.e. 3667 views (the cap and the knob TMI_BA_ROTATION_MAX_ORDER of the rotation estimator):
 * TMI_BA_ERR_UNSUPPORTED above it, before anything of the views' size is allocated, on the host (the connectivity
 * check included: a graph above the cap is refused whether connected or not) or on the device.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: a null batch, options, view_position or summary, a
 * missing array, num_pairs == 0, a view index out of range, view1 == view2, a repeated unordered pair, fixed_view out of
 * range, a non-finite rotation or position_2, rho, alpha or a tolerance that is not positive and finite,
 * max_num_iterations < 1 (the reference CHECK_GTs it), and a view that the edges do not connect to fixed_view.
 * On every failure view_position and the optional outputs are left as they were.  Optional outputs (each may be NULL):
 * pair_scale [num_pairs] the final s_e; pair_residual [3 * num_pairs] the final A x of the L1 rows; admm_r_norm /
 * admm_s_norm [max_num_iterations] the two norms of every iteration run. */
int32_t tmi_ba_estimate_global_positions_lud(const tmi_ba_view_pair_batch* batch,
                                             const tmi_ba_lud_position_options* options, int32_t fixed_view,
                                             int32_t device, double* view_position, double* pair_scale,
                                             double* pair_residual, double* admm_r_norm, double* admm_s_norm,
                                             tmi_ba_lud_position_summary* summary);

/* ---- NonlinearPositionEstimator: camera positions by Levenberg-Marquardt on the direction error ----
 * reference: nonlinear_position_estimator.cc:86-214 (GlobalPositionEstimatorType::NONLINEAR, the default of
 * ReconstructionEstimatorOptions, reconstruction_estimator_options.h:90; Wilson and Snavely, ECCV 2014) with
 * pairwise_translation_error.h:63-88 and Ceres 1.14's TrustRegionMinimizer, LevenbergMarquardtStrategy, HuberLoss and
 * Corrector.  max_num_iterations and robust_loss_width are NonlinearPositionEstimator::Options
 * (nonlinear_position_estimator.h:70-72); the trust-region fields are Ceres' Solver::Options defaults, which the
 * reference leaves alone. */
typedef struct tmi_ba_nonlinear_position_options {
  int32_t  max_num_iterations;                 /* 400; 0: the start is evaluated and returned              */
  double   robust_loss_width;                  /* 0.1, HuberLoss                                            */
  int32_t  positions_given;                    /* 0; != 0: view_position holds the start (EXTENSION)        */
  uint64_t seed;                               /* 0; of the random start                                    */
  int32_t  jacobi_scaling;                     /* 1                                                         */
  int32_t  max_num_consecutive_invalid_steps;  /* 5                                                         */
  double   function_tolerance;                 /* 1e-6                                                      */
  double   gradient_tolerance;                 /* 1e-10                                                     */
  double   parameter_tolerance;                /* 1e-8                                                      */
  double   initial_trust_region_radius;        /* 1e4                                                       */
  double   max_trust_region_radius;            /* 1e16                                                      */
  double   min_trust_region_radius;            /* 1e-32                                                     */
  double   min_relative_decrease;              /* 1e-3                                                      */
  double   min_lm_diagonal;                    /* 1e-6                                                      */
  double   max_lm_diagonal;                    /* 1e32                                                      */
} tmi_ba_nonlinear_position_options;
void tmi_ba_nonlinear_position_options_init(tmi_ba_nonlinear_position_options* options);

typedef struct tmi_ba_nonlinear_position_summary {
  int32_t num_views;
  int32_t num_pairs;
  int32_t num_iterations;           /* LM iterations run (one ended by the gradient test is not counted)       */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;   /* rejected and invalid steps                                              */
  int32_t num_factorizations;       /* dense Cholesky factorisations of order 3 (num_views - 1)                */
  int32_t termination;              /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE                              */
  int32_t usable;                   /* Summary::IsSolutionUsable(): termination != FAILURE                     */
  double  initial_cost;
  double  final_cost;
  double  seconds;
  double  kernel_seconds;           /* device time; the sum of the three below                                 */
  double  factor_seconds;           /* the damped copy of the normal matrix and its factorisation              */
  double  substitution_seconds;     /* forward / backward substitution                                         */
  double  graph_seconds;            /* directions, per-edge and per-view kernels, assembly, the reductions     */
} tmi_ba_nonlinear_position_summary;

/* EstimatePositions on the device.  The batch is tmi_ba_view_pair_batch: view_rotation (or NULL: pair_position2 is
 * already in the global frame), pair_view1 / pair_view2 and pair_position2; pair_rotation2 is not read.
 * view_position [3 * num_views] is in/out: the start when options->positions_given, the result afterwards; view
 * `fixed_view` is at 0.
 *   1. :59-66, :196-199  t_e = R(view_rotation[view1])^T position_2, step 1 of tmi_ba_estimate_global_positions_lud and
 *                its kernel.
 *   2. :164-180  The start.  positions_given: the caller's view_position.  Otherwise component k of view v is
 *                100 (2 u - 1) with u = ((word >> 11) + 0.5) 2^-53 and word = word 3 v + k of the splitmix64 stream from
 *                state `seed` (word c is the output mix of seed + (c + 1) 0x9e3779b97f4a7c15, the generator documented
 *                at the translation filter).  DEVIATION: not the reference's stream (100 RandVector3d() of its
 *                mt19937).  :131-132  view `fixed_view` is set to 0 and held constant; DEVIATION: the reference fixes
 *                whichever view its hash map yields first.  Free view v has columns 3 (v - (v > fixed_view)) + k;
 *                n = num_views - 1.
 *   3. pairwise_translation_error.h:63-88 (weight 1)  d = p[view2] - p[view1], norm = sqrt((d0 d0 + d1 d1) + d2 d2),
 *                norm = 1 where norm < 1e-12; u = d / norm; r = u - t_e.  The Jacobian with respect to p[view2] is what
 *                the reference's dual numbers give, J = (I - u u^T) / norm, and J = I on the small-norm branch (the
 *                derivative of the discarded norm is discarded with it); with respect to p[view1] it is -J.
 *   4. :201-207  HuberLoss(a = robust_loss_width) on s = (r0 r0 + r1 r1) + r2 r2 (ceres/loss_function.cc): s <= a^2:
 *                rho = s, rho' = 1, rho'' = 0; otherwise rho = 2 a sqrt(s) - a^2, rho' = max(DBL_MIN, a / sqrt(s)),
 *                rho'' = -rho' / (2 s).  Ceres' Corrector (corrector.cc), as the engine's robust path applies it: where
 *                s = 0 or rho'' <= 0 (the shortcut) r~ = sqrt(rho') r and J~ = sqrt(rho') J; otherwise
 *                alpha = 1 - sqrt(1 + 2 s rho'' / rho'), r~ = sqrt(rho') / (1 - alpha) r and
 *                J~ = sqrt(rho') (J - (alpha / s) r (r^T J)).  Triggs' correction would have alpha in [0, 1) for
 *                rho'' < 0 and clamp it below 1; Ceres takes alpha = 0 there instead, which is the shortcut.  HuberLoss
 *                never leaves it (rho'' <= 0 on both branches), so the shortcut is all the kernels carry.
 *                cost = sum of rho(s) / 2 over the edges.
 *   5.           The normal equations of order 3 n: with B_e = J~^T J~ and q_e = J~^T r~ the diagonal blocks of view1 and
 *                view2 get +B_e, block (view1, view2) is -B_e, the gradient gets +q_e at view2 and -q_e at view1; the
 *                fixed view's rows and columns are absent.  Jacobi scaling (jacobi_scaling != 0): column i is scaled
 *                by 1 / (1 + sqrt(the diagonal entry i at the start)), once.
 *   6.           Ceres 1.14's TrustRegionMinimizer with the Levenberg-Marquardt strategy, the rules of
 *                tmi_ba_solver_solve: per iteration (A + D) y = g with D_ii = clamp(A_ii, min_lm_diagonal,
 *                max_lm_diagonal) / radius by ONE dense Cholesky factorisation and one substitution, step = -scale y;
 *                a non-positive pivot or a model cost change -(J~ step) . (r~ + J~ step / 2) that is not positive is an
 *                invalid step (max_num_consecutive_invalid_steps in a row: FAILURE), which divides the radius by the
 *                decrease factor (2, doubling with every step in a row that is not accepted); then the parameter
 *                tolerance |step| <= parameter_tolerance (|x| + parameter_tolerance) and the function tolerance
 *                |cost change| <= function_tolerance cost end the solve with CONVERGENCE before the step is taken; a step
 *                with cost change / model cost change > min_relative_decrease is accepted, the radius divided by
 *                max(1/3, 1 - (2 rho - 1)^3) and capped at max_trust_region_radius; any other is rejected as an invalid
 *                one shrinks.  A radius below min_trust_region_radius and, after the first linearisation and after
 *                every accepted step, max |gradient| <= gradient_tolerance are CONVERGENCE.  A rejected or invalid step
 *                re-factors the kept normal matrix with the new diagonal; nothing is evaluated or assembled again.
 *   7.           Fixed orders: edges in the caller's order; every per-view sum from zero in ascending edge index;
 *                every scalar (cost, model cost change, the squared norms of the step and of x over their 3 n entries) by
 *                the reduction of fixed shape of step 5 of the LUD call; no expression is contracted into FMA and no
 *                atomic is used.  The result is the same bits from call to call.
 * The loop runs on the host; every kernel is a plain grid launch.  The call returns TMI_BA_OK whenever the solve ran:
 * summary->termination says how it ended and summary->usable is IsSolutionUsable (:161); view_position receives the
 * last accepted point in every case.
 * DEVIATIONS beyond steps 2: the linear solve is always the exact dense factorisation -- the reference takes
 * SPARSE_NORMAL_CHOLESKY up to 1000 views, the same step up to rounding, and CGNR with JACOBI above, an inexact step
 * (:139-157).  3 n is capped as in the rotation and the LUD call (11000, the knob TMI_BA_ROTATION_MAX_ORDER):
 * TMI_BA_ERR_UNSUPPORTED above it, before anything of that size is allocated.  The point-to-camera constraints
 * (min_num_points_per_view > 0, :216-361) are not provided: the reference's default and its application flag are 0.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: a null batch, options, view_position or summary, a
 * missing array, num_pairs == 0, a view index out of range, view1 == view2, a repeated unordered pair, fixed_view out of
 * range, a non-finite rotation or position_2, robust_loss_width that is not positive and finite (:93),
 * max_num_iterations < 0, a radius, tolerance or LM diagonal bound that is negative or NaN, an initial radius of 0,
 * positions_given with a non-finite position, and a view that the edges do not connect to fixed_view.
 * On every failure view_position and the optional outputs are left as they were.  Optional outputs (each may be NULL):
 * initial_position [3 * num_views] the start (the fixed view at 0); iteration_cost, iteration_radius and
 * iteration_step_accepted [max_num_iterations + 1]: entry 0 the initial cost, the initial radius and 1, entry k the cost
 * and the radius after iteration k and its outcome -- 1 accepted, 0 rejected, -1 invalid, 2 / 3 ended by the parameter /
 * the function tolerance; pair_residual [3 * num_pairs] the r of step 3 at the result. */
int32_t tmi_ba_estimate_global_positions_nonlinear(const tmi_ba_view_pair_batch* batch,
                                                   const tmi_ba_nonlinear_position_options* options,
                                                   int32_t fixed_view, int32_t device, double* view_position,
                                                   double* initial_position, double* iteration_cost,
                                                   double* iteration_radius, int32_t* iteration_step_accepted,
                                                   double* pair_residual,
                                                   tmi_ba_nonlinear_position_summary* summary);

/* ---- NonlinearRotationEstimator: global orientations by Levenberg-Marquardt on the relative rotation error ----
 * reference: nonlinear_rotation_estimator.cc:49-100 (GlobalRotationEstimatorType::NONLINEAR,
 * global_reconstruction_estimator.cc:335-339, hybrid_reconstruction_estimator.cc:329-334) with
 * pairwise_rotation_error.h:65-95 and Ceres 1.14's TrustRegionMinimizer, LevenbergMarquardtStrategy, SoftLOneLoss,
 * Corrector and rotation.h.  robust_loss_width is the constructor's (nonlinear_rotation_estimator.h, default 0.1),
 * max_num_iterations is :94; the trust-region fields are Ceres' Solver::Options defaults, which the reference leaves
 * alone. */
typedef struct tmi_ba_nonlinear_rotation_options {
  int32_t  max_num_iterations;                 /* 200; 0: the start is evaluated and returned              */
  double   robust_loss_width;                  /* 0.1, SoftLOneLoss                                         */
  int32_t  fixed_view;                         /* -1: no view is held, the reference's problem; >= 0: that
                                                  view is held constant (EXTENSION)                         */
  int32_t  jacobi_scaling;                     /* 1                                                         */
  int32_t  max_num_consecutive_invalid_steps;  /* 5                                                         */
  double   function_tolerance;                 /* 1e-6                                                      */
  double   gradient_tolerance;                 /* 1e-10                                                     */
  double   parameter_tolerance;                /* 1e-8                                                      */
  double   initial_trust_region_radius;        /* 1e4                                                       */
  double   max_trust_region_radius;            /* 1e16                                                      */
  double   min_trust_region_radius;            /* 1e-32                                                     */
  double   min_relative_decrease;              /* 1e-3                                                      */
  double   min_lm_diagonal;                    /* 1e-6                                                      */
  double   max_lm_diagonal;                    /* 1e32                                                      */
} tmi_ba_nonlinear_rotation_options;
void tmi_ba_nonlinear_rotation_options_init(tmi_ba_nonlinear_rotation_options* options);

typedef struct tmi_ba_nonlinear_rotation_summary {
  int32_t num_views;                /* views in the problem: marked, with an edge that is used                 */
  int32_t num_pairs;                /* edges used: both views marked                                           */
  int32_t num_iterations;           /* LM iterations run (one ended by the gradient test is not counted)       */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;   /* rejected and invalid steps                                              */
  int32_t num_factorizations;       /* dense Cholesky factorisations of order 3 (free views)                   */
  int32_t termination;              /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE                              */
  int32_t usable;                   /* Summary::IsSolutionUsable(): termination != FAILURE                     */
  double  initial_cost;
  double  final_cost;
  double  seconds;
  double  kernel_seconds;           /* device time; the sum of the three below                                 */
  double  factor_seconds;           /* the damped copy of the normal matrix and its factorisation              */
  double  substitution_seconds;     /* forward / backward substitution                                         */
  double  graph_seconds;            /* per-edge and per-view kernels, assembly, the reductions                 */
} tmi_ba_nonlinear_rotation_summary;

/* EstimateRotations on the device.  The batch is tmi_ba_view_pair_batch: num_views, pair_view1 / pair_view2 and
 * pair_rotation2 are read; the batch's view_rotation and pair_position2 are not.  view_rotation [3 * num_views],
 * angle-axis, is in/out and always the start: the reference refuses to run without an initialisation (:53-57).
 * view_given [num_views] (NULL: every view) marks the views that have one, the keys of the reference's map.
 *   1. :69-88    The problem.  An edge with an unmarked view is skipped (:76-80); the edges used keep the caller's order
 *                (DEVIATION: the reference walks its hash map).  The views of the problem are the marked views with an
 *                edge that is used, in ascending index; every other view is never written.  options->fixed_view = -1 is
 *                the reference's problem: every such view is free and nothing holds the gauge, the three-dimensional
 *                null space of the normal matrix is lifted by the LM diagonal alone.  fixed_view >= 0 (EXTENSION) holds
 *                that view constant and removes its rows and columns; a held view that is not in the problem holds
 *                nothing.  n = the number of free views, column c is the c-th of them.
 *   2. pairwise_rotation_error.h:65-95 (weight 1)  With R1, R2, Rrel = AngleAxisToRotationMatrix of x[view1], x[view2]
 *                and rotation_2, r = RotationMatrixToAngleAxis(R2 R1^T Rrel^T).  The 3 x 6 Jacobian is what forward-mode
 *                dual numbers give through Ceres' rotation.h, every branch taken on the values as the Jets take it:
 *                theta^2 > DBL_EPSILON or the first-order matrix I + [x] in AngleAxisToRotationMatrix (an exactly zero
 *                rotation, which the spanning tree's root carries, has the non-zero derivatives of [x]); trace >= 0 or
 *                the largest diagonal entry (first of equals) in RotationMatrixToQuaternion; sin^2 > 0 or k = 2, and
 *                atan2(-sin, -cos) for a negative scalar part, in QuaternionToAngleAxis.  Jet division is by the inverse
 *                of the divisor's value, sqrt' = 1 / (2 sqrt), atan2(g, f)' = (f g' - g f') / (f^2 + g^2).
 *   3. :66-67    SoftLOneLoss(a = robust_loss_width) on s = (r0 r0 + r1 r1) + r2 r2 (ceres/loss_function.cc), b = a^2:
 *                rho = 2 b (sqrt(1 + s / b) - 1), rho' = max(DBL_MIN, 1 / sqrt(1 + s / b)),
 *                rho'' = -1 / (2 b (1 + s / b)^(3/2)).  Ceres' Corrector takes the shortcut r~ = sqrt(rho') r,
 *                J~ = sqrt(rho') J where s = 0 or rho'' <= 0 (step 4 of tmi_ba_estimate_global_positions_nonlinear gives
 *                the other case); SoftLOneLoss has rho'' < 0 everywhere, so the shortcut is all the kernels carry.
 *                cost = sum of rho(s) / 2 over the edges used.
 *   4.           The normal equations of order 3 n: with J1~, J2~ the halves of J~ for view1 and view2 -- independent, not
 *                +-J as in the position call -- the diagonal block of view1 gets J1~^T J1~, that of view2 J2~^T J2~, block
 *                (view1, view2) J1~^T J2~ and the gradient J1~^T r~ at view1, J2~^T r~ at view2; a held view's rows and
 *                columns are absent.  Jacobi scaling as in step 5 of the position call.
 *   5.           Steps 6 and 7 of tmi_ba_estimate_global_positions_nonlinear word for word: the kept normal matrix and a
 *                damped copy factored per trial radius, the invalid / rejected / accepted step rules, the three
 *                tolerances, the fixed orders (edges in the caller's order, per-view sums in ascending edge index, every
 *                scalar by the reduction of fixed shape), no FMA contraction, no atomics, the same bits from call to call.
 *                The code is shared.
 * The loop runs on the host; every kernel is a plain grid launch.  TMI_BA_OK whenever the solve ran; summary->termination
 * says how it ended; view_rotation receives the last accepted point in every case (a held view's and every view's outside
 * the problem bit for bit as given).  Marked views but no edge between two of them: TMI_BA_OK, an empty problem, nothing
 * written (the reference solves an empty problem and returns true).
 * THE GAUGE.  With fixed_view = -1 the result is defined up to one rotation applied to every view of a connected
 * component, and rounding in the gradient's gauge component is amplified by up to radius / A_ii: two correct
 * implementations agree in the loop rotations R2 R1^T, the residuals, the costs and the radii, not in view_rotation itself.
 * DEVIATIONS beyond step 1: the linear solve is always the dense factorisation (the reference: SPARSE_NORMAL_CHOLESKY, the
 * same step up to rounding); 3 n is capped as in the position call (11000, the knob TMI_BA_ROTATION_MAX_ORDER):
 * TMI_BA_ERR_UNSUPPORTED above it, before anything of that size is allocated.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: the reference's two refusals (its `false`) -- num_pairs == 0
 * or no marked view -- and a null batch, options, view_rotation or summary, a missing array, a view index out of range,
 * view1 == view2, a repeated unordered pair, a non-finite rotation_2 or marked view_rotation, fixed_view outside
 * [-1, num_views) or unmarked, robust_loss_width that is not positive and finite, max_num_iterations < 0, a radius,
 * tolerance or LM diagonal bound that is negative or NaN, an initial radius of 0.
 * On every failure view_rotation and the optional outputs are left as they were.  Optional outputs (each may be NULL):
 * iteration_cost, iteration_radius and iteration_step_accepted [max_num_iterations + 1] as in the position call;
 * pair_residual [3 * num_pairs] the r of step 2 at the result, 0 for a skipped edge. */
int32_t tmi_ba_estimate_global_rotations_nonlinear(const tmi_ba_view_pair_batch* batch,
                                                   const tmi_ba_nonlinear_rotation_options* options,
                                                   const uint8_t* view_given, int32_t device, double* view_rotation,
                                                   double* iteration_cost, double* iteration_radius,
                                                   int32_t* iteration_step_accepted, double* pair_residual,
                                                   tmi_ba_nonlinear_rotation_summary* summary);

/* ---- LinearRotationEstimator: global orientations as the three smallest eigenvectors of a block Laplacian ----
 * reference: linear_rotation_estimator.cc:78-203 (GlobalRotationEstimatorType::LINEAR,
 * global_reconstruction_estimator.cc:340-344; Martinec and Pajdla, CVPR 2007) with ProjectToRotationMatrix
 * (pose/util.cc:121-133).  max_iterations and tolerance are Spectra's defaults maxit and tol, which the reference leaves
 * alone.  The only rotation estimator that needs no initialisation. */
typedef struct tmi_ba_linear_rotation_options {
  int32_t  max_iterations;   /* 1000                                                                        */
  double   tolerance;        /* 1e-10: the stop rule's residual, relative to 2 x the largest degree         */
  double   relative_shift;   /* 1e-9: M + mu I is factored, mu = relative_shift x the largest degree        */
  uint64_t seed;             /* 0: the start block's splitmix64 stream                                      */
} tmi_ba_linear_rotation_options;
void tmi_ba_linear_rotation_options_init(tmi_ba_linear_rotation_options* options);

typedef struct tmi_ba_linear_rotation_summary {
  int32_t num_views;             /* views in the problem: those with an edge                                */
  int32_t num_pairs;
  int32_t order;                 /* 3 num_views, the order of the matrix                                    */
  int32_t num_iterations;        /* subspace iterations run                                                 */
  int32_t converged;             /* the stop rule was met within max_iterations                             */
  int32_t usable;                /* 0: a pivot of M + mu I was not positive; nothing was written            */
  int32_t num_reflected;         /* views whose projection was negated (determinant < 0)                    */
  double  eigenvalue[4];         /* the three Ritz values of the result and the fourth, ascending           */
  double  residual[3];           /* |M q - theta q|_2 of the three Ritz pairs                               */
  double  seconds;
  double  kernel_seconds;        /* device time; the sum of the three below                                 */
  double  factor_seconds;        /* the factorisation of M + mu I                                           */
  double  substitution_seconds;  /* forward / backward substitution on the block of 6                       */
  double  graph_seconds;         /* assembly, M Q, Gram-Schmidt, Rayleigh-Ritz, the reductions, projection  */
} tmi_ba_linear_rotation_summary;

/* EstimateRotations on the device.  The batch is tmi_ba_view_pair_batch: num_views, pair_view1 / pair_view2 and
 * pair_rotation2 are read; the batch's view_rotation and pair_position2 are not.  view_rotation [3 * num_views],
 * angle-axis, is written only: there is no start.  The views of the problem are those with an edge, in ascending index
 * (the order of the matrix is n = 3 x their number); every other view's view_rotation is never written.
 *   1. :90-152   M, symmetric of order n: with R12 = AngleAxisToRotationMatrix(rotation_2) every edge adds I3 to both
 *                diagonal blocks, -R12^T at block (view1, view2) and -R12 at block (view2, view1): the matrix of
 *                sum |X2 - R12 X1|_F^2 over 3 x 3 blocks X_i.  Its diagonal is the views' degrees.
 *   2. :173-181  The three eigenvectors of the smallest eigenvalues.  The reference: Spectra shift-invert Lanczos at
 *                sigma = 0 on a sparse LL^T of M itself.  HERE (DEVIATION): subspace iteration with Rayleigh-Ritz on a
 *                block of 6 columns (the reference's ncv) through one dense Cholesky factorisation of M + mu I,
 *                mu = relative_shift x the largest degree.  The shift moves every eigenvalue by mu and no eigenvector; it
 *                makes the noise-free problem, whose M is exactly singular, factorable.
 *                Start block Q [n][6]: Q[i][j] = 2 u - 1, u = ((word >> 11) + 0.5) 2^-53, word 6 i + j of the splitmix64
 *                stream from state `seed` (the generator documented at tmi_ba_localize_views).
 *                Each iteration: Y = (M + mu I)^-1 Q; Y orthonormalised by modified Gram-Schmidt, two passes;
 *                T = Y^T (M Y) with M applied from the edge list, not from the factor; T = W diag(theta) W^T by cyclic
 *                Jacobi (12 sweeps over the pairs (0,1) (0,2) .. (4,5), theta ascending, the first of equals first, every
 *                column of W signed so that its coefficient of largest magnitude, the first of equals, is positive);
 *                Q = Y W.  Stop when |M q_j - theta_j q_j|_2 <= tolerance x 2 x the largest degree (Gershgorin's bound on
 *                the largest eigenvalue) for j = 0, 1, 2, or after max_iterations.
 *   3. :188-200  Per view the 3 x 3 block of rows of the first three columns of Q is projected to SO(3): U V^T of its
 *                SVD (one-sided Jacobi), negated when the determinant is negative, then RotationMatrixToAngleAxis.  A
 *                block of rank two is completed by the cross product of its two left vectors; one of lower rank gives a
 *                finite value that is no rotation (the reference's is arbitrary there too).
 * THE GAUGE.  The result is defined up to one rotation G applied on the right of every view's matrix, R_i G, and which G
 * comes out depends on rounding wherever two of the three eigenvalues are close: two correct implementations agree in
 * the loop rotations R_j R_i^T, not in view_rotation itself.  num_reflected is 0 or num_views unless the noise is gross.
 * Fixed orders, no FMA contraction, no atomics: the same bits from call to call.  The loop runs on the host; every kernel
 * is a plain grid launch.
 * TMI_BA_OK whenever the solve ran: summary->converged and ->usable say how; the last Ritz vectors are projected and
 * written unless usable == 0.  TMI_BA_ERR_UNSUPPORTED when n exceeds the dense solver's cap (11000, the knob
 * TMI_BA_ROTATION_MAX_ORDER), before anything of that size is allocated.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: a null batch, options, view_rotation or summary,
 * num_pairs == 0 (the reference CHECK_GTs its constraints), a missing array, a view index out of range, view1 == view2,
 * a repeated unordered pair, a non-finite rotation_2, max_iterations <= 0, a tolerance that is not positive and finite,
 * a relative_shift that is negative or not finite, and (DEVIATION) view pairs that are not connected: with c components
 * the null space has 3 c dimensions and the three smallest eigenvectors mix the components; the reference returns
 * garbage there and its pipeline runs RemoveDisconnectedViewPairs first.
 * On every failure view_rotation is left as it was. */
int32_t tmi_ba_estimate_global_rotations_linear(const tmi_ba_view_pair_batch* batch,
                                                const tmi_ba_linear_rotation_options* options, int32_t device,
                                                double* view_rotation, tmi_ba_linear_rotation_summary* summary);

/* ---- ExtractMaximallyParallelRigidSubgraph: the largest set of views whose positions the edges fix up to scale ----
 * reference: extract_maximally_parallel_rigid_subgraph.cc:53-228 (Kennedy, Daniilidis, Naroditsky and Taylor, IROS 2012;
 * the first step of FilterRelativeTranslation with extract_maximal_rigid_subgraph,
 * global_reconstruction_estimator.cc:382-387). */
typedef struct tmi_ba_rigid_subgraph_options {
  double  relative_shift;      /* 1e-9: L + mu I is factored, mu = relative_shift x the largest diagonal entry of L  */
  double  null_tolerance;      /* 1e-9: a Ritz value <= null_tolerance x the largest diagonal entry is null          */
  int32_t max_null_dimension;  /* 128 (the hard cap): a larger null space is TMI_BA_ERR_NULL_SPACE_TOO_LARGE         */
  int32_t max_iterations;      /* 100: block iterations over all block widths                                       */
  int32_t device;              /* -1: the current device                                                            */
} tmi_ba_rigid_subgraph_options;
void tmi_ba_rigid_subgraph_options_init(tmi_ba_rigid_subgraph_options* options);

typedef struct tmi_ba_rigid_subgraph_summary {
  int32_t num_views;             /* views of the problem: those with an edge inside the mask                 */
  int32_t num_pairs;             /* edges of the problem                                                     */
  int32_t order;                 /* n = 3 num_views                                                          */
  int32_t null_dimension;        /* k                                                                        */
  int32_t block_width;           /* m of the last block: 8, 16, ... 128                                      */
  int32_t iterations;            /* block iterations over all widths                                         */
  int32_t fixed_view;            /* the fixed view of the component that won (the caller's index; -1: none)  */
  int32_t num_kept;              /* views with keep = 1                                                      */
  double  largest_diagonal;      /* of L: what both tolerances are relative to                               */
  double  stop_tolerance;        /* 1e-3 x null_tolerance x largest_diagonal                                 */
  double  max_residual;          /* the largest |L q_j - theta_j q_j|_2 of the null pairs                    */
  double  largest_null_value;    /* the Ritz values on both sides of the cut                                 */
  double  smallest_other_value;  /* (0 where the block holds no such pair)                                   */
  double  seconds;
  double  kernel_seconds;        /* device time; the sum of the four below                                   */
  double  factor_seconds;        /* the matrix and the factorisation of L + mu I                             */
  double  substitution_seconds;  /* forward / backward substitution on the block                             */
  double  graph_seconds;         /* L Y, Gram-Schmidt, Rayleigh-Ritz, the reductions                         */
  double  search_seconds;        /* the rows of M, the pair sweep, the count and the pick                    */
} tmi_ba_rigid_subgraph_summary;

/* ExtractMaximallyParallelRigidSubgraph on the device.  The batch is tmi_ba_view_pair_batch: view_rotation (the
 * orientations), pair_view1 / pair_view2 and pair_position2 are read; pair_rotation2 is not.  view_mask [num_views]
 * (NULL: every view): 0 = the view and its edges are not there.  The views of the problem are those with an edge
 * between two views of the mask, in ascending index; n = 3 x their number.
 *   1. :61-84    Per edge d = R(orientation of view1)^T position_2 (Ceres' AngleAxisToRotationMatrix) and C = [d]x; the
 *                edge's rows of the measurement matrix A are [-C at view1, +C at view2].
 *   2. :196-197  L = A^T A, of order n: C^T C = |d|^2 I - d d^T is added to both diagonal blocks of the edge (a view's
 *                sum runs in the caller's edge order) and -C^T C is the block between its views.  A is never formed.
 *   3. :196-198  N [n][k], a basis of the null space of L.  The reference: the kernel of a full-pivot LU.  HERE
 *                (DEVIATION): an orthonormal basis by block inverse iteration with Rayleigh-Ritz through one dense
 *                Cholesky factorisation of L + mu I.  The block has m = 8 columns (start: 2 u - 1, u from word m i + c of
 *                the splitmix64 stream of state 0); an iteration is Y = (L + mu I)^-1 Q, modified Gram-Schmidt in
 *                column order (two passes), T = Y^T (L Y) with L applied from the edge list, T = W diag(theta) W^T by
 *                cyclic Jacobi (16 sweeps in round-robin order), Q = Y W.  A pair is null when
 *                theta <= null_tolerance x largest_diagonal.  When all m pairs are null, m doubles and the iteration
 *                starts over; past max_null_dimension (or 128) that is TMI_BA_ERR_NULL_SPACE_TOO_LARGE, so a null space
 *                is only accepted below the block's width.  Stop when the null count is below m, unchanged, and every
 *                null pair's residual |L q - theta q|_2 is <= stop_tolerance, for two iterations in a row.
 *                Step 4 does not depend on the basis: parallel rows stay parallel under any invertible change of it.
 *   4. :104-168  For every fixed view f: M = N - replicate(N_f), the row norms, the rows normalised (a row of norm 0 is
 *                left alone), in that order.  A view i != f is a zero view when its three norms are < 1e-10.  Views i, j
 *                are parallel when both are neither f nor zero views and 1 - |<M_i,d, M_j,d>| < 1e-5 for d = x, y, z.  The
 *                component of f is f, every zero view, and every view that is parallel to at least one other view.
 *   5. :207-227  The largest component wins, the smallest f among equals.
 * keep [num_views]: 1 for the views of that component, 0 for every other view -- also (DEVIATION) for a view without an
 * edge or outside the mask, which is no part of the system here; the reference sizes its matrix by the orientation map,
 * gives such a view three zero columns, hence three more null directions, and keeps it as a zero view.
 * component_size [num_views] (optional): the size of the component found with each view fixed, 0 outside the problem.
 * null_space (optional; room for 3 num_views x max_null_dimension doubles): N, [order][null_dimension] row major over
 * the problem's views, every column signed so that its entry of largest magnitude, the first of equals, is positive.
 * Fixed orders, no FMA contraction, no atomics: the same bytes from call to call.
 * Argument checks, in this order, all TMI_BA_ERR_INVALID_ARGUMENT before the device is looked for: a null batch,
 * options, keep or summary; the batch (negative size, a missing array, more than 2^30 pairs, a view index out of range,
 * view1 == view2, a repeated unordered pair, a non-finite orientation or position_2); relative_shift negative or not
 * finite; null_tolerance not positive and finite; max_null_dimension outside [1, 128]; max_iterations <= 0.  Then
 * TMI_BA_ERR_UNSUPPORTED when n exceeds the dense solver's cap (11000, the knob TMI_BA_ROTATION_MAX_ORDER), before
 * anything of that size is allocated; TMI_BA_ERR_NO_DEVICE; a device that does not exist (INVALID_ARGUMENT).  From the
 * device: TMI_BA_ERR_LINEAR_SOLVER (a pivot of L + mu I is not positive, or every direction is zero),
 * TMI_BA_ERR_NOT_CONVERGED (max_iterations), TMI_BA_ERR_NULL_SPACE_TOO_LARGE.  A problem without an edge is
 * TMI_BA_OK with keep all 0.  On every failure keep, component_size and null_space are left as they were; the summary
 * holds what was known. */
int32_t tmi_ba_extract_parallel_rigid_subgraph(const tmi_ba_view_pair_batch* batch, const uint8_t* view_mask,
                                               const tmi_ba_rigid_subgraph_options* options, uint8_t* keep,
                                               int32_t* component_size, double* null_space,
                                               tmi_ba_rigid_subgraph_summary* summary);

/* ---- LinearPositionEstimator: global positions as the smallest eigenvector of the view triplets' constraints ----
 * reference: linear_position_estimator.cc:163-470 (GlobalPositionEstimatorType::LINEAR_TRIPLET; Jiang, Cui and Tan,
 * ICCV 2013) with TripletExtractor (math/graph/triplet_extractor.h), FindCommonTracksInViews and
 * ComputeTripletBaselineRatios (compute_triplet_baseline_ratios.cc:55-156).  The only position estimator that needs no
 * start, and the only pose estimator here that reads the tracks.  max_iterations and tolerance are Spectra's defaults. */
typedef struct tmi_ba_linear_position_options {
  int32_t  max_iterations;   /* 1000                                                                        */
  double   tolerance;        /* 1e-10: the stop rule's residual, relative to |M|_inf                        */
  double   relative_shift;   /* 1e-9: M + mu I is factored, mu = relative_shift x the largest diagonal entry */
  uint64_t seed;             /* 0: the start block's splitmix64 stream                                      */
  double   min_triangulation_angle_degrees; /* 2.0: kMinTriangulationAngle, compute_triplet_baseline_ratios.cc:60 */
} tmi_ba_linear_position_options;
void tmi_ba_linear_position_options_init(tmi_ba_linear_position_options* options);

typedef struct tmi_ba_linear_position_summary {
  int32_t num_views;                 /* of the batch                                                        */
  int32_t num_pairs;
  int32_t num_triplets;              /* triangles of the view graph                                         */
  int32_t num_triplets_with_baseline;/* those with at least one usable common track                         */
  int32_t num_triplet_components;    /* components of the triplets with a baseline                          */
  int32_t num_chosen_triplets;       /* triplets of the chosen component                                    */
  int32_t num_chosen_views;          /* views of the chosen component: the estimated views                  */
  int32_t triplets_written;          /* 1: triplet_capacity sufficed and the optional arrays were written   */
  int64_t num_dropped_ratios;        /* common tracks dropped for a ratio that is not finite and positive   */
  int32_t order;                     /* 3 (num_chosen_views - 1), the order of the matrix                   */
  int32_t num_iterations;            /* subspace iterations run                                             */
  int32_t converged;                 /* the stop rule was met within max_iterations                         */
  int32_t usable;                    /* 0: no triplet with a baseline, or a pivot of M + mu I was not positive;
                                        nothing was written                                                 */
  double  eigenvalue[2];             /* the Ritz value of the result and the next                           */
  double  residual;                  /* |M q - theta q|_2 of the result                                     */
  double  matrix_norm;               /* |M|_inf, the largest absolute row sum                               */
  int32_t sign_votes;                /* the integer sum of the votes, before any flip                       */
  int32_t flipped;                   /* 1: the sum was negative and every position was negated              */
  double  seconds;
  double  kernel_seconds;            /* device time; the sum of the five below                              */
  double  triplet_seconds;           /* triangle count, scan and fill                                       */
  double  baseline_seconds;          /* features, common tracks, triangulations and the order statistics    */
  double  factor_seconds;            /* the factorisation of M + mu I                                       */
  double  substitution_seconds;      /* forward / backward substitution on the block of 6                   */
  double  graph_seconds;             /* components, records, assembly, M Y, Gram-Schmidt, Rayleigh-Ritz, the vote */
} tmi_ba_linear_position_summary;

/* EstimatePositions on the device.  The problem supplies the camera model and intrinsics of every view (camera i is view
 * i of the batch: num_cameras == num_views) and all observations (view, track, pixel), as tmi_ba_localize_views reads
 * them; extrinsics, points and the estimated flags are not consulted (FindCommonTracksInViews does not consult them).
 * Of the batch pair_view1 / pair_view2 (view1 < view2), pair_rotation2, pair_position2 and view_rotation (the global
 * orientations) are read.  view_position [3 * num_views] and view_estimated [num_views] are written on success:
 * view_estimated is 1 for the views of the chosen triplet component and 0 for every other view, whose position is never
 * written.  The optional arrays (each may be NULL) have room for triplet_capacity triplets: triplet_view [3 *] the
 * views a < b < c, triplet_pair [3 *] the batch indices of the pairs (a, b), (a, c), (b, c), triplet_baseline [3 *]
 * (0, 0, 0 where there is none), triplet_num_common, triplet_num_used, triplet_component (the smallest triplet of the
 * component, -1 for a triplet without a baseline).  With a capacity below summary->num_triplets none of them is
 * written, summary->triplets_written is 0, and the solve runs all the same.
 *   1. triplet_extractor.h:166-226   Every triangle of the view graph once, as (a < b < c), numbered in lexicographic
 *                order (DEVIATION: the reference's order is that of its hash sets).  One wavefront per edge (a, b)
 *                intersects the two sorted adjacency rows for c > b: a count pass, a scan, a fill pass.
 *   2. :423-430, compute_triplet_baseline_ratios.cc:110-112   Per observation, once: the feature is
 *                PixelToNormalizedCoordinates(pixel), then hnormalized(), then homogeneous().normalized().
 *   3. compute_triplet_baseline_ratios.cc:55-156   Per triplet the common tracks of the three views (the views' track
 *                lists are sorted; every track of the first is looked up in the other two).  Per common track three
 *                two-view triangulations, origins {0, position_2}, directions {f1, R2^T f2}, R2 =
 *                AngleAxisToRotationMatrix(rotation_2): SufficientTriangulationAngle at
 *                min_triangulation_angle_degrees, then TriangulateMidpoint.  The track counts only if all three succeed;
 *                its ratios are depth1_12 / depth1_13 and depth2_12 / depth2_23.  The baseline is (1, r2[m], r3[m]),
 *                r[m] the element of index count / 2 of the sorted ratios, what nth_element leaves there.  The selection
 *                is exact for any count: by rank counting in LDS where the shortest of the three track lists has at most
 *                1024 tracks, in per-triplet scratch in global memory otherwise.
 *                DEVIATION: a track with a ratio that is not finite and positive is dropped and counted
 *                (num_dropped_ratios); the reference would hand a NaN to nth_element.
 *                DEVIATION: a triplet with no usable track is removed here; the reference leaves its baseline at zero
 *                and the NaN that follows poisons the whole matrix.
 *   4. triplet_extractor.h:232-259, :67-84   The components of the triplets that survived step 3 (DEVIATION in order: the
 *                reference forms them before it knows the baselines): two triplets are joined when they share a view
 *                PAIR; sharing one view does not join them.  Union-find with the smaller root kept.  The largest
 *                component wins, between equals the one with the smallest triplet number (the reference's std::sort on
 *                sizes leaves this open).  No surviving triplet: TMI_BA_OK, usable = 0, nothing written.
 *   5. :230-248, :295-421   The views of the chosen component in ascending index are the unknowns and the first of them is
 *                held at the origin (DEVIATION: the reference holds whichever view its hash order meets first; with noise
 *                the answer depends on this choice).  w = 1 / sqrt(the fewest chosen triplets any of the three views is
 *                in).  Per triplet: t_ij = -R_i^T position_2 with R_i = AngleAxisToRotationMatrix(view_rotation[i])
 *                (Ceres' formula, DEVIATION: the reference's Eigen::AngleAxisd divides by a zero angle), the three
 *                rotations Quaterniond::FromTwoVectors(..).toRotationMatrix() by Eigen's formula (DEVIATION: where the two
 *                vectors are within 1e-12 of antiparallel Eigen takes an axis from an SVD; here the rotation is by pi
 *                about normalized(v0 x e_k), e_k the coordinate axis of v0's smallest |component|, the first of equals),
 *                the three scale ratios and the nine 3 x 3 constraint blocks, kept as one record per triplet.  The matrix
 *                is M = A^T A, dense, of order n = 3 (V' - 1), rows and columns of the held view left out; a block (i, j)
 *                is the sum over the triplets with both views in ascending triplet number, one writer per block.
 *   6. :195-208  The eigenvector of the smallest eigenvalue.  The reference: Spectra, 1 wanted, ncv 6, sigma 0.  HERE
 *                (DEVIATION): the subspace iteration of tmi_ba_estimate_global_rotations_linear, step 2 there, with the
 *                same block of 6 columns, start, Gram-Schmidt, Jacobi order and sign rule, through one dense Cholesky
 *                factorisation of M + mu I, mu = relative_shift x the largest diagonal entry of M.  M Y is applied from
 *                the triplet records as A^T (A Y), never from the factor.  Stop when |M q_0 - theta_0 q_0|_2 <=
 *                tolerance x |M|_inf, the largest absolute row sum, or after max_iterations.  The noise-free problem has
 *                eigenvalue exactly 0: the shift is what makes it factorable.  A pivot that is not positive: usable = 0,
 *                nothing written.
 *   7. :210-222, :432-470   A free view takes its segment of q_0 (|q_0| = 1 over the free views), the held view 0.  Then
 *                the vote over every batch edge whose two views are both estimated: +1 where
 *                AngleAxisRotatePoint(view_rotation[view1], normalized(p2 - p1)) . position_2 > 0 and -1 otherwise; all
 *                positions are negated when the integer sum is negative.
 * Fixed orders, no floating-point atomics, no FMA contraction in the new kernels: the same bytes from call to call.
 * TMI_BA_ERR_UNSUPPORTED when n exceeds the dense solver's cap (11000, the knob TMI_BA_ROTATION_MAX_ORDER) before
 * anything of that size is allocated, and for more than 2^30 triplets.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: a null problem, batch, options, view_position,
 * view_estimated or summary, num_pairs == 0, a missing array, num_cameras != num_views, a bad intrinsics group or
 * observation index, a view that observes a track twice, a view index out of range, pair_view1 >= pair_view2 (the
 * reference's ViewIdPair keys are ordered and its look-ups for a sorted triplet rely on that), a repeated pair, a
 * non-finite rotation_2, position_2 or orientation of a view with an edge, max_iterations <= 0, a tolerance that is not
 * positive and finite, a negative or non-finite relative_shift, a triangulation angle outside (0, 180), a negative
 * triplet_capacity.  On every failure the outputs are left as they were. */
int32_t tmi_ba_estimate_global_positions_linear(const tmi_ba_problem* problem, const tmi_ba_view_pair_batch* batch,
                                                const tmi_ba_linear_position_options* options, int32_t device,
                                                double* view_position, uint8_t* view_estimated,
                                                int32_t triplet_capacity, int32_t* triplet_view, int32_t* triplet_pair,
                                                double* triplet_baseline, int32_t* triplet_num_common,
                                                int32_t* triplet_num_used, int32_t* triplet_component,
                                                tmi_ba_linear_position_summary* summary);

/* ---- batched LocalizeViewToReconstruction: P3P RANSAC for many candidate views ------------------
 * reference: LocalizeViewToReconstruction (localize_view_to_reconstruction.cc:213-257), the inner loop of the
 * incremental and hybrid pipelines (incremental_reconstruction_estimator.cc:219-233), on its CALIBRATED path:
 * EstimateCameraPose with known intrinsics and without assume_known_orientation (:185-198),
 * EstimateCalibratedAbsolutePose with RansacType::RANSAC (estimate_calibrated_absolute_pose.cc:58-110),
 * SampleConsensusEstimator::Estimate (sample_consensus_estimator.h:246-344) with InlierSupport, and PoseFromThreePoints
 * (perspective_three_point.cc).  Not provided: P4Pf (unknown focal length), the known-orientation position solver,
 * use_mle, use_Tdd_test, PROSAC, LMED and exhaustive sampling.
 * The problem holds the candidate views as cameras; EVERY point of the problem counts as an estimated track; view_mask
 * [num_cameras] selects the candidates (NULL = all); the input extrinsics of a selected view are ignored.
 * view_error_threshold [num_cameras] is RansacParameters::error_thresh per view: the SQUARED threshold in normalised
 * coordinates (:188-191), i.e. (ComputeResolutionScaledThreshold(pixels, width, height) / focal_length)^2, which the
 * caller computes because tmi_ba_problem has no image size.  Per selected view, in this order:
 *   1. Correspondences: the view's observations in ascending observation index, numbered 0..n-1; the feature is
 *      Camera::PixelToNormalizedCoordinates(pixel).hnormalized() (as step 2 of tmi_ba_estimate_tracks, all five
 *      models), the world point is point.hnormalized().  n < min_num_inliers (:141-145)        -> status 1.
 *      (Also n < 3: the reference's sampler refuses to initialise.)
 *   2. The sample of iteration i.  samples_given != 0: the caller's samples[3 (max_iterations v + i) + k], v the camera
 *      index.  Otherwise deterministic in `seed` and stateless: word c = 3 (v 2^32 + i) + k (mod 2^64) of the splitmix64
 *      stream from state `seed` (the generator documented at tmi_ba_filter_view_pairs_from_relative_translation: the
 *      state after c + 1 steps is seed + (c + 1) gamma and the word is the output mix of that state),
 *      u = ((word >> 11) + 0.5) 2^-53, j_k = min(k + floor(u (n - k)), n - 1), then the three swaps of a partial
 *      Fisher-Yates on the identity permutation, swap(a[k], a[j_k]) for k = 0, 1, 2; the sample is a[0..2].
 *      THE SAMPLE SEQUENCES ARE NOT THE REFERENCE'S: its RandomSampler carries its permutation from one iteration to the
 *      next and draws from another generator.
 *   3. P3P as PoseFromThreePoints writes it: the collinearity test (< 1e-6), the swap when intermediate_image_point[2]
 *      > 0, the quartic in cos(theta), cot(alpha) and the back-substitution with its sign rules, then position = -R^T t.
 *      The reference takes the roots from the companion matrix and back-substitutes THE REAL PART OF EVERY ONE OF THE FOUR
 *      ROOTS, complex ones included; so does this call: four solutions per sample, in ascending real part (a conjugate
 *      pair gives the same pose twice).  The roots come from Ferrari's factorisation through a positive root of the
 *      resolvent cubic found by bisection, with two Newton steps on every real root.  A leading coefficient of exactly
 *      0 gives no model (DEVIATION: the reference would drop the degree).
 *   4. The cost of a solution: the correspondences whose squared reprojection error
 *      |hnormalized(R (X - c)) - feature|^2 is not below the threshold (a NaN error is an outlier), the three sampled
 *      ones included.
 *   5. The replay in ascending (iteration, solution) order, exactly the loop at sample_consensus_estimator.h:276-330: a
 *      solution becomes the best on cost < best_cost, strictly; inlier_ratio < 3 / n skips the update of the bound;
 *      max_iterations = min(ComputeMaxIterations(3, inlier_ratio, log(failure_probability)), max_iterations) with the
 *      reference's formula (its - epsilon, its inlier_ratio == 1 case, its clamp between min_iterations and
 *      max_iterations); the initial bound comes from min_inlier_ratio when that is positive (:268-274); a sample without
 *      a model still counts as an iteration; the loop ends when the iteration counter reaches the current bound.
 *      Iterations are evaluated on the device in chunks of chunk_iterations (0: max(min_iterations, 64)); what a chunk
 *      evaluated beyond the end of the loop is discarded, so THE RESULT DOES NOT DEPEND ON chunk_iterations.
 *   6. Final (:332-341): the inlier mask of the best model, num_inliers its count, confidence =
 *      1 - (1 - (num_inliers / n)^3)^num_iterations.  No solution in any iteration -> status 2 (DEVIATION: the reference
 *      goes on with an uninitialised model).  num_inliers < min_num_inliers (:239) -> status 3.
 *   7. Otherwise the view is localised: problem->extrinsics of the view becomes the position and the orientation as
 *      Camera::SetOrientationFromRotationMatrix sets it (Ceres' RotationMatrixToAngleAxis).  With bundle_adjust_view the
 *      batched view adjustment (tmi_ba_adjust_views with ba_options) then runs on exactly the localised views, on the
 *      data already on the device; a view whose adjustment is not usable gets status 4 and keeps its RANSAC pose (the
 *      reference has set the pose and SetEstimated(true) by then, :247-252, and returns false).  Otherwise status 0.
 * view_status: -1 not selected, 0..4 as above.  Every per-view output [num_cameras] may be NULL.  view_best_iteration /
 * view_best_solution: the (iteration, solution) of the best model, -1 without one.  obs_inlier [num_observations]
 * (optional): 1 for the inliers of the best model of an attempted view, 0 elsewhere.  hypothesis_cost
 * [num_selected * max_iterations * 4] (optional, for tests; selected views in ascending camera index): the cost of every
 * replayed hypothesis, -1 for no model or not replayed.
 * With samples_given the whole table [3 * max_iterations * num_cameras] is uploaded, the rows of views that are not
 * attempted included (12 bytes per camera and iteration).
 * ComputeMaxIterations and the confidence are evaluated on the host (log and pow of the C library); steps 2 to 6 use
 * + - * / and sqrt only and are never contracted into FMA.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device (ba_options->device) is looked for: a null problem, options, ba_options
 * or summary, a missing array, a bad index or intrinsics group, the CHECKs of the SampleConsensusEstimator constructor
 * (an error threshold of an attempted view that is not positive, min_inlier_ratio outside [0, 1], failure_probability
 * outside (0, 1), max_iterations < min_iterations), a negative count, max_iterations above 2^20, samples_given without
 * samples, and a sample of an attempted view with a repeated or out-of-range index. */
typedef struct tmi_ba_localization_options {
  double   failure_probability;  /* 0.01 (sample_consensus_estimator.h:57-65)                                  */
  double   min_inlier_ratio;     /* 0                                                                          */
  int32_t  min_iterations;       /* 100                                                                        */
  int32_t  max_iterations;       /* 1000; the reference's struct default is INT_MAX, its estimators set
                                    ransac_max_iterations                                                      */
  int32_t  min_num_inliers;      /* 30 (localize_view_to_reconstruction.h:71)                                  */
  int32_t  bundle_adjust_view;   /* 1                                                                          */
  int32_t  chunk_iterations;     /* 0 = the engine's choice                                                    */
  uint64_t seed;                 /* 0                                                                          */
} tmi_ba_localization_options;
void tmi_ba_localization_options_init(tmi_ba_localization_options* options);

typedef struct tmi_ba_localization_summary {
  int32_t num_views;                    /* selected views                                   */
  int32_t num_localized;                /* status 0                                         */
  int32_t num_too_few_correspondences;  /* status 1                                         */
  int32_t num_no_model;                 /* status 2                                         */
  int32_t num_too_few_inliers;          /* status 3                                         */
  int32_t num_failed_ba;                /* status 4                                         */
  int32_t num_chunks;                   /* chunks of iterations evaluated                   */
  int64_t total_iterations;             /* RANSAC iterations over the attempted views       */
  double  seconds;
  double  kernel_seconds;               /* the RANSAC launches, first to last (the per-chunk read-back of the done flags
                                           included), plus the view adjustment's           */
} tmi_ba_localization_summary;

int32_t tmi_ba_localize_views(tmi_ba_problem* problem, const tmi_ba_localization_options* options,
                              const tmi_ba_options* ba_options, const uint8_t* view_mask,
                              const double* view_error_threshold, const int32_t* samples, int32_t samples_given,
                              int8_t* view_status, int32_t* view_num_correspondences, int32_t* view_num_inliers,
                              int32_t* view_num_iterations, int32_t* view_best_iteration, int32_t* view_best_solution,
                              double* view_confidence, uint8_t* obs_inlier, int32_t* hypothesis_cost,
                              tmi_ba_localization_summary* summary);

/* ---- batched BruteForceFeatureMatcher: exact squared-L2 descriptor matching for many image pairs ---
 * reference: BruteForceFeatureMatcher::MatchImagePair (brute_force_feature_matcher.cc:49-117) with IntersectMatches
 * (feature_matcher_utils.cc:48-71) and the defaults of FeatureMatcherOptions (feature_matcher_options.h:45-71).  Not
 * provided: geometric verification, the databases (cascade hashing: tmi_ba_match_features_cascade below).  A one-shot call without a tmi_ba_problem; THE
 * DESCRIPTORS AND DISTANCES ARE fp32 (the one exception to this header's fp64 rule), as the reference's are.
 * Image m owns the descriptor rows image_begin[m] .. image_begin[m + 1] - 1 of `descriptors` [rows x dim, row-major];
 * every image goes to the device once however many pairs name it.  Per pair (image1, image2), N1 and N2 rows:
 *   1. Distance, in fp32: acc = 0; for k = 0 .. dim-1 ascending: t = a[k] - b[k]; acc = acc + t * t -- every
 *      subtraction, multiplication and addition rounded on its own (no FMA, no reassociation), subnormals kept.  This is
 *      the reference's (a - b).squaredNorm() with the summation order fixed (Eigen leaves it open).  d(a, b) == d(b, a).
 *   2. Forward pass: for every row i of image 1 the best and the second-best column of image 2 under the total order
 *      (distance, then LOWER COLUMN INDEX; the reference's partial_sort leaves ties open).  A NaN distance never wins.
 *   3. Ratio test as the reference types it (:58-59, :79): ratio_sq = (double)(float)(lowes_ratio * lowes_ratio), the
 *      product formed in fp32; row i passes when (double)d0 < ratio_sq * (double)d1.  Without use_lowes_ratio every row
 *      passes if N2 >= 1.  With it and N2 < 2 no row passes (DEVIATION: the reference reads past the end there).
 *   4. pair_num_forward = the rows that passed.  Fewer than min_num_feature_matches (:84-86): status 1, no matches.
 *   5. With keep_only_symmetric_matches the same pass with the roles swapped; the forward match (i, j) survives when
 *      the reverse pass kept a match for row j of image 2 whose best column is i.  Then the count is tested against
 *      min_num_feature_matches again (:116): fewer -> status 1, no matches.  (The reverse pass of a pair that failed
 *      step 4 is still computed; nothing of it is visible.)
 *   6. Otherwise status 0 and the matches in ascending feature1 index: (feature1, feature2, distance), the distance the
 *      fp32 value of the forward pass.
 * Empty images, N = 1, a pair of an image with itself and duplicate descriptors follow from these rules.  Non-finite
 * descriptor values are the caller's error and are not validated.
 * Outputs: pair_status [num_pairs] (0 ok, 1 too few matches), pair_num_forward [num_pairs], pair_match_begin
 * [num_pairs + 1] (int64; the matches of pair p are pair_match_begin[p] .. pair_match_begin[p + 1] - 1), and
 * match_feature1 / match_feature2 / match_distance [match_capacity].  When match_capacity is smaller than the total,
 * the call returns TMI_BA_ERR_CAPACITY with the needed total in summary->num_matches; the three per-pair arrays are
 * filled all the same and the match arrays are unspecified, so the caller can size them and call again.
 * Pairs are processed in chunks of consecutive pairs whose work memory (34 bytes per descriptor row and direction: the
 * neighbour triple, two flags, the scan and the compacted match) stays within a fixed budget; pairs_per_chunk > 0 sets
 * the number of pairs of a chunk instead.
 * THE RESULT DOES NOT DEPEND ON THE CHUNKING, nor on anything else about how the device is driven: steps 1 to 6 leave
 * nothing open.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device (options->device) is looked for: a null options or summary, a missing
 * array, a negative count, dim < 1, image_begin that does not start at 0 or decreases, an image index out of range,
 * a negative min_num_feature_matches or pairs_per_chunk, an image of 2^31 - 1 rows or more.  TMI_BA_ERR_UNSUPPORTED:
 * a single pair whose rows exceed what a chunk can index (2^31 - 1 over both directions). */
typedef struct tmi_ba_match_options {
  int32_t use_lowes_ratio;              /* 1                                        */
  float   lowes_ratio;                  /* 0.8f                                     */
  int32_t keep_only_symmetric_matches;  /* 1                                        */
  int32_t min_num_feature_matches;      /* 30                                       */
  int32_t device;                       /* -1 = the current device                  */
  int32_t pairs_per_chunk;              /* 0 = from the work-memory budget          */
} tmi_ba_match_options;
void tmi_ba_match_options_init(tmi_ba_match_options* options);

typedef struct tmi_ba_match_summary {
  int64_t num_matches;           /* over all pairs (the needed match_capacity)                                   */
  int64_t distance_evaluations;  /* N1 N2 per pair and direction                                                  */
  int32_t num_pairs_ok;          /* status 0                                                                      */
  int32_t num_chunks;
  double  kernel_seconds;        /* the chunks' launches, first to last of each chunk                             */
  double  total_seconds;
} tmi_ba_match_summary;

int32_t tmi_ba_match_features(const tmi_ba_match_options* options, int32_t num_images, const int64_t* image_begin,
                              const float* descriptors, int32_t dim, int32_t num_pairs, const int32_t* pair_image1,
                              const int32_t* pair_image2, int64_t match_capacity, int8_t* pair_status,
                              int32_t* pair_num_forward, int64_t* pair_match_begin, int32_t* match_feature1,
                              int32_t* match_feature2, float* match_distance, tmi_ba_match_summary* summary);

/* ---- batched CascadeHashingFeatureMatcher: hashed shortlists, exact distances on eleven columns per row ----
 * reference: CascadeHasher (cascade_hasher.cc:55-277; Cheng et al., CVPR 2014) and
 * CascadeHashingFeatureMatcher::MatchImagePair (cascade_hashing_feature_matcher.cc:130-166), the matcher the
 * reference's applications run by default (--matching_strategy=CASCADE_HASHING).  Not provided: the LRU cache of hashed
 * images (a call hashes every image once), AddImage(s), geometric verification, the databases.  A one-shot call
 * without a tmi_ba_problem; descriptors, projections and distances are fp32.  The images, the pairs, the outputs and
 * the TMI_BA_ERR_CAPACITY protocol are those of tmi_ba_match_features.
 * `projections` [188 x dim, row-major] is an INPUT (the reference draws it from a clock-seeded generator, so there is
 * nothing reproducible to restate; theia::CascadeHashingFeatureMatcher draws it from a seed): rows 0..127 are the
 * primary projection (kHashCodeSize 128), row 128 + 10 g + k is bit k of bucket group g (kNumBucketGroups 6,
 * kNumBucketBits 10; cascade_hasher.h:52-58).
 *   1. Mean (:55-62), per image with N >= 1 rows, in fp32: for every dimension k, m = 0; for i = 0 .. N-1 ascending:
 *      m = m + x[i][k]; then m = m / (float)N.
 *   2. Projection (:94-117), per row and projection row r, in fp32: t[k] = x[k] - m[k]; acc = 0; for k ascending:
 *      acc = acc + P[r][k] * t[k] -- every operation rounded on its own (no FMA), subnormals kept.  The bit is acc > 0.
 *      Code bit j is the bit of row j; the bucket id of group g is the sum over k of bit(128 + 10 g + k) << (9 - k).
 *      DEVIATION of the kind of step 1 of tmi_ba_match_features: Eigen leaves the summation order of its
 *      matrix-vector product open; this fixes it.
 *   3. Candidates of row i of image 1 in image 2 (:206-226): column c is a candidate of group g when
 *      bucket2[c][g] == bucket1[i][g].  total = the number of (c, g) incidences, duplicates counted.  total <= 10: the
 *      row has no match (the reference's `<= kNumTopCandidates`).
 *   4. Shortlist (:228-260): among the UNIQUE candidates the 11 smallest under the total order (Hamming distance of
 *      the 128-bit codes, first group g in which c is a candidate, column index c), all of them if there are fewer.
 *      This is exactly the reference's walk over its Hamming bins in insertion order with the buckets filled in
 *      ascending index: a bin holds its columns in the order they were first met, i.e. by (first group, column), and
 *      the walk stops once it holds more than ten.  total > 10 implies at least two unique candidates (a column
 *      counts at most six times), so the reference's partial_sort(begin, begin + 2, end) is always in range.
 *   5. Exact distances of the shortlisted columns by step 1 of tmi_ba_match_features (the same bits: (b - a)^2 equals
 *      (a - b)^2); the best and the second best under (distance, then lower column), which is std::pair<float, int>'s
 *      own operator<.
 *   6. Ratio test as the reference types it (:180, :268-271, cascade_hashing_feature_matcher.cc:144-145):
 *      sq = (double)lowes_ratio * (double)lowes_ratio, or 1.0 without use_lowes_ratio; the row is dropped when
 *      (double)d0 > (double)d1 * sq.  (NOT step 3 of tmi_ba_match_features: `>` against `<`, the square in double.)
 *   7. Counts and intersection (cascade_hashing_feature_matcher.cc:152-165): steps 4 to 6 of tmi_ba_match_features --
 *      the forward count against min_num_feature_matches, with keep_only_symmetric_matches the reverse pass and
 *      IntersectMatches, the count again, the matches in ascending feature1 with the forward d0.
 *   8. An empty image has no hash and no matches (:144-146, :175-177); its pairs' rows are not counted as skipped.
 * THE RESULT DOES NOT DEPEND ON THE CHUNKING, the grid, the thread mapping or the physical order of a bucket: steps 1
 * to 8 leave nothing open.
 * Test outputs, each may be null: image_hash [rows x 4 uint32: code bit j is bit j % 32 of word j / 32] and
 * image_bucket_ids [rows x 6 uint16].
 * summary: distance_evaluations counts the exact distances of step 5 only; candidates_examined the incidences
 * (`total`) of the rows that were not skipped and rows_skipped the rows that failed step 3, both over every pass that
 * is computed (the reverse pass whenever keep_only_symmetric_matches is set); kernel_seconds includes the hashing.
 * TMI_BA_ERR_INVALID_ARGUMENT as for tmi_ba_match_features, and for a null `projections`. */
typedef struct tmi_ba_cascade_match_options {
  int32_t use_lowes_ratio;              /* 1                                        */
  float   lowes_ratio;                  /* 0.8f                                     */
  int32_t keep_only_symmetric_matches;  /* 1                                        */
  int32_t min_num_feature_matches;      /* 30                                       */
  int32_t device;                       /* -1 = the current device                  */
  int32_t pairs_per_chunk;              /* 0 = from the work-memory budget          */
} tmi_ba_cascade_match_options;
void tmi_ba_cascade_match_options_init(tmi_ba_cascade_match_options* options);

typedef struct tmi_ba_cascade_match_summary {
  int64_t num_matches;           /* over all pairs (the needed match_capacity)                                   */
  int64_t distance_evaluations;  /* exact distances (step 5)                                                      */
  int32_t num_pairs_ok;          /* status 0                                                                      */
  int32_t num_chunks;
  double  kernel_seconds;        /* the hashing launches plus the chunks' launches, first to last of each        */
  double  total_seconds;
  int64_t candidates_examined;   /* candidate incidences of the rows that were not skipped                       */
  int64_t rows_skipped;          /* rows with total <= 10                                                         */
} tmi_ba_cascade_match_summary;

int32_t tmi_ba_match_features_cascade(const tmi_ba_cascade_match_options* options, int32_t num_images,
                                      const int64_t* image_begin, const float* descriptors, int32_t dim,
                                      const float* projections, int32_t num_pairs, const int32_t* pair_image1,
                                      const int32_t* pair_image2, int64_t match_capacity, int8_t* pair_status,
                                      int32_t* pair_num_forward, int64_t* pair_match_begin, int32_t* match_feature1,
                                      int32_t* match_feature2, float* match_distance, uint32_t* image_hash,
                                      uint16_t* image_bucket_ids, tmi_ba_cascade_match_summary* summary);

/* ---- batched GuidedEpipolarMatcher: more matches along the epipolar lines of a known two-view geometry ----
 * reference: GuidedEpipolarMatcher (matching/guided_epipolar_matcher.{h,cc}; line numbers below are the .cc's), the
 * step of TwoViewMatchGeometricVerification::VerifyMatches (two_view_match_geometric_verification.cc:157-167) between
 * the pose estimate and the triangulation.  A one-shot call without a tmi_ba_problem for many image pairs, shaped like
 * tmi_ba_match_features: image m owns the rows image_begin[m] .. image_begin[m + 1] - 1 of `descriptors` [rows x dim,
 * fp32, row-major] and of `keypoints` [rows x 2, fp64: x, y]; every image that a selected pair names goes to the
 * device once however many pairs name it (summary->rows_uploaded).  Pair p is (pair_image1[p], pair_image2[p]) with
 * fundamental_matrix [9 p .. 9 p + 8], row-major, which maps a point of image 1 to its line in image 2, and the input
 * matches pair_match_begin[p] .. pair_match_begin[p + 1] - 1 of match_feature1 / match_feature2 (row indices local to
 * the two images).  pair_mask (optional): a pair with pair_mask[p] == 0 is not computed, its status is -1 and it adds
 * nothing.  pair_stream (optional): the random stream q of pair p (default q = p), so that a pair computed alone
 * repeats what it gave in a batch.  Per selected pair, N1 and N2 rows, c = guided_matching_max_distance_pixels:
 *   a. Matched sets (:102-142).  A feature of either image that occurs in an input match is matched.  The box
 *      (top_left, bottom_right) is the minimum and the maximum of x and of y over the UNMATCHED features of image 2.
 *      No unmatched feature in image 2, or none in image 1: status 1, nothing added, no groups.
 *   b. Epipolar lines (:214-236), per unmatched feature (x, y) of image 1, in fp64 with + - * / sqrt only, every
 *      operation rounded on its own (no FMA): l_r = (F[3r] x + F[3r + 1] y) + F[3r + 2] for r = 0, 1, 2; n =
 *      sqrt(l_0 l_0 + l_1 l_1); l_r = l_r / n.  The intersections of FindEpipolarLineIntersection (:320-356) in its
 *      order: left (tl.x, -(l_2 + l_0 tl.x) / l_1), top (-(l_2 + l_1 tl.y) / l_0, tl.y), right (br.x, -(l_2 + l_0
 *      br.x) / l_1), bottom (-(l_2 + l_1 br.y) / l_0, br.y); each is kept when its free coordinate v satisfies
 *      v >= low && v <= high of the box with IEEE comparisons (a NaN or an infinity fails, which is how the reference
 *      treats vertical and horizontal lines).  Exactly two kept intersections are the endpoints, otherwise the
 *      feature is skipped.  Each of the four coordinates is truncated toward zero.  DEVIATION: the reference casts to
 *      uint16_t, undefined outside its range; here a truncated coordinate outside [0, 65535] skips the feature.
 *      code = x1 << 48 | y1 << 32 | x2 << 16 | y2 (:60-71).
 *   c. Groups (:239-273).  The features that were not skipped, sorted by (code, feature index) ascending (the order
 *      std::sort gives the reference's pairs).  In that order: the decoded endpoints e0 = (x1, y1), e1 = (x2, y2) as
 *      doubles; a new group (endpoints E0 = e0, E1 = e1, no features) starts at the first feature and whenever
 *      (E0.x - e0.x)^2 + (E0.y - e0.y)^2 > c c, E0 the current group's running first endpoint; then the feature joins
 *      the current group, w = 1.0 / (number of its features), and E0 = (1.0 - w) E0 + w e0, E1 = (1.0 - w) E1 + w e1
 *      per coordinate.  Groups are numbered from 0 in this order.  The scan is sequential by definition.
 *   d. Four grids (:108-113, :438-480) of cell size 2 c with offsets (0, 0), (c, 0), (0, c), (c, c).  The cell centre
 *      of a point in the grid of offset (ox, oy): (int)(((floor((x - ox) / (2.0 c)) * 2.0) * c + c) + ox), the same in
 *      y with oy, truncated toward zero.  A cell holds the UNMATCHED features of image 2 with that centre.  (Centres
 *      are assumed to fit an int32, as in the reference.)
 *   e. Candidates of a group (:284-318).  num_steps = (int)(sqrt(dx dx + dy dy) / c) with (dx, dy) = E1 - E0; delta =
 *      (E0 - E1) / (double)num_steps; s = E1; num_steps times: s = s + delta, then of the four centres of s the
 *      closest one, squared distance (cx - s.x)^2 + (cy - s.y)^2, strict < in grid order 0..3 (:416-436), and that
 *      cell's features join the candidate SET.  The set has no order (a bitmap over the N2 rows here).  With fewer
 *      than min_num_candidates members, draws t = |set| .. min_num_candidates - 1 insert a row of image 2, matched
 *      ones included, duplicates collapsing (:308-314).  DEVIATION: the reference draws from its own generator; here
 *      draw t is min((int)(u N2), N2 - 1), u = ((word >> 11) + 0.5) 2^-53, word number 64 (q 2^32 + g) + t of the
 *      splitmix64 stream of `seed` (the stream of the RANSAC calls), g the group's number.
 *   f. Search (:358-414, :172-184).  For every feature of the group the best and the second-best candidate under
 *      steps 1 and 2 of tmi_ba_match_features: fp32, t = a[k] - b[k], acc = acc + t * t for ascending k, no FMA, the
 *      total order (distance, then lower row index), a NaN distance never wins.  DEVIATION: the search is exact, where
 *      the reference asks an approximate FLANN kd-tree.  Fewer than two candidates: no match (DEVIATION: the reference
 *      reads past the end).  Ratio test as typed at :150, :177: (double)d0 < (double)d1 * (lowes_ratio * lowes_ratio),
 *      the square formed in double.  A passing feature adds (feature1, best row, d0).  The added matches of a pair
 *      come out in ascending (group, position in the group); nothing makes the image-2 side unique, as in the
 *      reference.
 * THE RESULT DOES NOT DEPEND ON HOW THE DEVICE IS DRIVEN: steps a to f leave nothing open.
 * Outputs: pair_status [num_pairs] (0 ok, 1 nothing to match, -1 masked out), pair_num_groups [num_pairs],
 * pair_added_begin [num_pairs + 1] (int64) and added_feature1 / added_feature2 / added_distance [added_capacity], the
 * distance the fp32 squared distance d0.  With added_capacity smaller than the total the call returns
 * TMI_BA_ERR_CAPACITY with the needed total in summary->num_added; the per-pair arrays and the test outputs are filled
 * all the same and nothing is written to the three added arrays.
 * Test outputs, each may be null; row(p) = the sum of N1 over the pairs before p, masked ones included:
 * feature_group [row(num_pairs)]: entry row(p) + i is the group number of feature i of image 1 in pair p, or -1;
 * group_endpoints [4 row(num_pairs)] and group_num_candidates [row(num_pairs)]: group g of pair p is entry row(p) + g
 * (E0.x, E0.y, E1.x, E1.y after the scan; the size of the candidate set after the fill); other entries are 0.
 * summary: num_pairs the selected pairs, num_groups, num_candidates (the set sizes summed over the groups),
 * distance_evaluations (set size times features, summed over the groups), rows_uploaded.
 * Limits: an image has at most 131072 rows (the candidate bitmap of a group is 16 KiB of LDS).  TMI_BA_ERR_UNSUPPORTED,
 * also before the device is looked for: 0 < c < 1/16 (c >= 1/16 bounds a walk at 2^21 steps); the rows of image 1
 * summed over the selected pairs, or four times those of image 2, reaching 2^31.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device (options->device) is looked for: a null options or summary, a missing
 * array, a negative count, dim < 1, image_begin that does not start at 0 or decreases, pair_match_begin likewise, an
 * image or match index out of range, c <= 0 or not finite, lowes_ratio not finite, min_num_candidates outside
 * [0, 64], an image of more than 131072 rows. */
typedef struct tmi_ba_guided_match_options {
  double   guided_matching_max_distance_pixels;  /* 2.0                                   */
  double   lowes_ratio;                          /* 0.8                                   */
  int32_t  min_num_candidates;                   /* 50 (kMinNumMatchesFound)              */
  int32_t  device;                               /* -1 = the current device               */
  uint64_t seed;                                 /* 0                                     */
  int32_t  reserved[2];                          /* 0                                     */
} tmi_ba_guided_match_options;
void tmi_ba_guided_match_options_init(tmi_ba_guided_match_options* options);

typedef struct tmi_ba_guided_match_summary {
  int64_t num_added;             /* over all pairs (the needed added_capacity)                                   */
  int64_t num_groups;
  int64_t num_candidates;        /* candidate set sizes after the fill, summed over the groups                   */
  int64_t distance_evaluations;  /* set size times group features, summed over the groups                        */
  int64_t rows_uploaded;         /* descriptor rows sent to the device: each named image once                    */
  int32_t num_pairs;             /* selected by the mask                                                          */
  int32_t num_pairs_ok;          /* status 0                                                                      */
  double  seconds;
  double  kernel_seconds;        /* first to last launch of the call                                              */
} tmi_ba_guided_match_summary;

int32_t tmi_ba_guided_epipolar_match(const tmi_ba_guided_match_options* options, int32_t num_images,
                                     const int64_t* image_begin, const float* descriptors, int32_t dim,
                                     const double* keypoints, int32_t num_pairs, const int32_t* pair_image1,
                                     const int32_t* pair_image2, const double* fundamental_matrix,
                                     const int64_t* pair_match_begin, const int32_t* match_feature1,
                                     const int32_t* match_feature2, const uint8_t* pair_mask,
                                     const uint32_t* pair_stream, int64_t added_capacity, int8_t* pair_status,
                                     int32_t* pair_num_groups, int64_t* pair_added_begin, int32_t* added_feature1,
                                     int32_t* added_feature2, float* added_distance, int32_t* feature_group,
                                     double* group_endpoints, int32_t* group_num_candidates,
                                     tmi_ba_guided_match_summary* summary);

/* ---- TrackBuilder: the tracks of a reconstruction from the verified matches of all view pairs, by union-find ----
 * reference: TrackBuilder (track_builder.cc:53-151) on ConnectedComponents<uint64_t> (connected_components.h:87-162),
 * driven from reconstruction_builder.cc:173,358,432-439 with the defaults of reconstruction_builder.h:81-85
 * (min_track_length 2, max_track_length 50).  Not provided: ViewGraph components, ReconstructionBuilder, the feature
 * and match databases, a resident form, coordinates as keys (theia::TrackBuilder owns the Feature-to-index map).  A
 * one-shot call without a tmi_ba_problem, all integers.
 * Input: E = num_edges correspondences; edge e joins the endpoints 2e and 2e + 1 of endpoint_view / endpoint_feature
 * [2E].  endpoint_feature is a feature index LOCAL TO ITS VIEW: the same index in two views names two features.
 *   1. Nodes (track_builder.cc:70-74, :133-151).  A node is a distinct (view, feature); its id is the rank of its first
 *      appearance among the 2E endpoints in ascending endpoint index -- the order of the reference's FindOrInsert ids.
 *   2. The components of the unconstrained graph: the partition union-find gives with no size cap.
 *   3. The cap (connected_components.h:87-108).  A component of at most max_track_length nodes is one set: the
 *      reference's loop never refuses a merge inside it, because the sizes of two of its parts sum to at most its
 *      size.  A larger component is REPLAYED: its edges in ascending edge index; an edge finds both roots and is skipped
 *      when they are equal or size1 + size2 > max_track_length (:94-97), otherwise the sets are united.  Only the
 *      partition matters, not which root survives (:101-107).  Components never interact in the reference's loop (a
 *      root's size and id change only by edges of its own component), so the replay per component gives exactly the
 *      reference's partition for its edge order.
 *   4. Labels and small sets.  A set's label is its smallest node id.  A set of fewer than min_track_length nodes is
 *      dropped and counted in num_small_tracks, before step 5 as in the reference (track_builder.cc:98).  DEVIATION: a
 *      set of one node is always dropped (and counted): with min_track_length <= 1 the reference reaches AddTrack with
 *      one observation and aborts (:121).
 *   5. Consistency (:107-119).  Among the nodes of an emitted set with the same view the lowest node id is kept, the
 *      others are counted in num_inconsistent_features.  DEVIATION: the reference keeps whichever its unordered_set
 *      iterates first.
 *   6. Output: the tracks in ascending label, a track's observations in ascending node id, as a CSR: track_begin
 *      [num_tracks + 1], obs_view / obs_feature [num_observations].  DEVIATION: the reference's order is its
 *      unordered_map's.
 * THE RESULT DOES NOT DEPEND ON HOW THE DEVICE IS DRIVEN: steps 1 to 6 leave nothing open, so whatever the grid, the
 * arrival order of atomics or any chunking, the outputs are the same bytes.
 * Capacity, the protocol of tmi_ba_match_features: track_begin has room for track_capacity + 1 entries, obs_view and
 * obs_feature for obs_capacity.  With either too small the call returns TMI_BA_ERR_CAPACITY, writes none of the three
 * and leaves the needed totals in summary->num_tracks and summary->num_observations (every other summary field and
 * the two test outputs are filled as well).
 * Test outputs, each may be null: endpoint_node [2E], the node id of every endpoint, and endpoint_label [2E], the label
 * of its final set, whether that set was emitted or dropped.
 * summary: num_sets = num_tracks + num_small_tracks; num_replayed_edges the edges of the oversize components;
 * kernel_seconds the device time of the four phases, phase_seconds: nodes / components / cap / output, each from a pair
 * of events around launches that are queued anyway.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for and with every output untouched: null options or
 * summary, a missing array (endpoint_view / endpoint_feature when E > 0, track_begin, obs_view / obs_feature when
 * obs_capacity > 0), a negative count, E >= 2^30, max_track_length < 1 (the reference's CHECK_GT,
 * connected_components.h:77), min_track_length < 1, an edge whose two endpoints have the same view (the reference's
 * CHECK_NE, track_builder.cc:66).  E = 0: TMI_BA_OK, zero tracks, track_begin[0] = 0.  Without a device:
 * TMI_BA_ERR_NO_DEVICE.  A loop bound reached on the device (never, by the argument in track_build_kernels.h):
 * TMI_BA_ERR_DEVICE. */
typedef struct tmi_ba_track_build_options {
  int32_t min_track_length;  /* 2                          */
  int32_t max_track_length;  /* 50                         */
  int32_t device;            /* -1 = the current device    */
} tmi_ba_track_build_options;
void tmi_ba_track_build_options_init(tmi_ba_track_build_options* options);

typedef struct tmi_ba_track_build_summary {
  int64_t num_nodes;
  int64_t num_components;
  int64_t num_oversize_components;
  int64_t num_replayed_edges;
  int64_t num_sets;
  int64_t num_tracks;                 /* the needed track_capacity */
  int64_t num_observations;           /* the needed obs_capacity   */
  int64_t num_small_tracks;
  int64_t num_inconsistent_features;
  double  seconds;
  double  kernel_seconds;
  double  phase_seconds[4];           /* nodes, components, cap, output */
} tmi_ba_track_build_summary;

int32_t tmi_ba_build_tracks(const tmi_ba_track_build_options* options, int64_t num_edges,
                            const uint32_t* endpoint_view, const uint32_t* endpoint_feature, int64_t track_capacity,
                            int64_t obs_capacity, int64_t* track_begin, uint32_t* obs_view, uint32_t* obs_feature,
                            uint32_t* endpoint_node, uint32_t* endpoint_label, tmi_ba_track_build_summary* summary);

/* ---- the view-graph steps between the edge filters and the global solvers ---------------------
 * reference: RemoveDisconnectedViewPairs (view_graph/remove_disconnected_view_pairs.cc:48-95; called after every
 * filtering step, global_reconstruction_estimator.cc:312, 366, 398) and OrientationsFromMaximumSpanningTree
 * (view_graph/orientations_from_maximum_spanning_tree.cc:109-180; the start RobustRotationEstimator is given,
 * global_reconstruction_estimator.cc:326-334).  Both take tmi_ba_view_pair_batch; only num_views, num_pairs, pair_view1
 * and pair_view2 are read, and pair_rotation2 by the orientations.  UNLIKE the filters a repeated unordered pair is
 * accepted.  pair_mask [num_pairs]: 0 = the edge is not there (already filtered); NULL = every edge is alive.
 *
 * tmi_ba_largest_connected_component:
 *   1. :52-59   Components over the alive edges.  view_label[v] is the smallest view index of v's component; a view
 *               without an alive edge is a component of its own (the reference never sees such a view).
 *   2. :61-69   The largest component is the one with the most views; AMONG EQUALS THE ONE WITH THE SMALLEST LABEL,
 *               where the reference takes the first its hash map yields.  Only components with at least one edge
 *               compete.  view_in_largest[v] = 1 for its views.
 *   3. :71-86   pair_keep[e] = 1 exactly for the alive edges inside the largest component (the edges
 *               RemoveView leaves in the graph).
 *   With no alive edge there is no component to keep: view_in_largest and pair_keep are all 0, largest_label = -1 and
 *   the call returns TMI_BA_OK (the reference's loops have nothing to remove).
 * summary: num_components counts the components with at least one edge; num_pairs_removed the alive edges outside the
 * largest component; num_views_removed the views of the OTHER components with at least one edge -- the size of the
 * set the reference returns.  Outputs, each may be NULL: view_label [num_views] int32, view_in_largest [num_views],
 * pair_keep [num_pairs].
 *
 * tmi_ba_orientations_from_maximum_spanning_tree, per call in this order:
 *   1. :114-119 The largest component as above.
 *   2. :121-136 The maximum spanning tree of that component by weight pair_num_verified_matches: exactly the tree the
 *               reference's Kruskal gives.  Its std::sort over pair<int, pair<ViewId, ViewId>>
 *               (math/graph/minimum_spanning_tree.h:83) is a total order, ascending (-num_verified_matches,
 *               min(view1, view2), max(view1, view2)) (a repeated pair: then the edge index); under a total order the
 *               minimum spanning tree is unique, and the device finds it by Boruvka rounds on the ranks of that order.
 *   3. :152     The root.  root_view == -1: the smallest view index of the largest component.  A NAMED ROOT where the
 *               reference takes mst.begin()->first of a hash set.  A root outside the largest component:
 *               TMI_BA_ERR_INVALID_ARGUMENT, every output untouched.
 *   4. :62-84   The root's orientation is 0.  Every other view of the tree gets ComputeOrientation from its tree
 *               parent: Ceres' AngleAxisToRotationMatrix of the parent's orientation and of the edge's pair_rotation2,
 *               R_rel R_parent when the parent is pair_view1 of the edge and R_rel^T R_parent when it is pair_view2,
 *               Ceres' RotationMatrixToAngleAxis -- the conversion at every step, as in the reference.  A view's value
 *               depends on its parent's alone, so the reference's heap order (:149-178) does not matter.
 * Outputs, each may be NULL: view_orientation [3 * num_views] (views outside the tree ARE LEFT AS THEY WERE),
 * view_parent, view_parent_pair, view_depth [num_views] int32 (-1 for the root's parent and parent pair and for every
 * view outside the tree; the root's depth is 0), pair_in_tree [num_pairs].
 * No alive edge: TMI_BA_OK, summary->usable = 0, num_tree_pairs = 0 and no array written (the reference returns false,
 * minimum_spanning_tree.h:71-74).  Otherwise usable = 1 and num_tree_pairs = largest_num_views - 1.
 *
 * Both calls: all integer results go through integer atomics only, so two calls give the same bytes.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device is looked for: a null batch or summary, a missing array, negative
 * counts, a view index out of range, a pair of a view with itself, a negative num_verified_matches on an alive edge,
 * root_view outside [-1, num_views).  Without a device: TMI_BA_ERR_NO_DEVICE.  A loop bound reached on the device, or a
 * tree that does not span the component (never, by the argument in view_graph_kernels.h): TMI_BA_ERR_DEVICE.  ON EVERY
 * FAILURE EVERY OUTPUT, THE SUMMARY INCLUDED, IS LEFT AS IT WAS. */
typedef struct tmi_ba_view_graph_component_summary {
  int32_t num_components;     /* components with at least one edge               */
  int32_t largest_label;      /* -1: no alive edge                               */
  int32_t largest_num_views;
  int32_t num_pairs_kept;
  int32_t num_pairs_removed;  /* alive edges outside the largest component       */
  int32_t num_views_removed;  /* views of the other components with an edge      */
  double  seconds;
  double  kernel_seconds;
} tmi_ba_view_graph_component_summary;

typedef struct tmi_ba_spanning_tree_summary {
  tmi_ba_view_graph_component_summary component;  /* seconds / kernel_seconds: of the whole call */
  int32_t num_tree_pairs;
  int32_t tree_depth;         /* the largest view_depth                          */
  int32_t root_view;          /* -1 when not usable                              */
  int32_t usable;             /* 0: no alive edge, nothing written               */
} tmi_ba_spanning_tree_summary;

int32_t tmi_ba_largest_connected_component(const tmi_ba_view_pair_batch* batch, const uint8_t* pair_mask,
                                           int32_t device, int32_t* view_label, uint8_t* view_in_largest,
                                           uint8_t* pair_keep, tmi_ba_view_graph_component_summary* summary);

int32_t tmi_ba_orientations_from_maximum_spanning_tree(const tmi_ba_view_pair_batch* batch,
                                                       const int32_t* pair_num_verified_matches,
                                                       const uint8_t* pair_mask, int32_t root_view, int32_t device,
                                                       double* view_orientation, int32_t* view_parent,
                                                       int32_t* view_parent_pair, int32_t* view_depth,
                                                       uint8_t* pair_in_tree, tmi_ba_spanning_tree_summary* summary);

/* ---- batched EstimateUncalibratedRelativePose: eight-point RANSAC for many uncalibrated view pairs -------
 * reference: the UNCALIBRATED branch of EstimateTwoViewInfo (estimate_twoview_info.cc:202-248), which the reference's
 * application runs for every view without an EXIF focal length: EstimateUncalibratedRelativePose with
 * RansacType::RANSAC (estimators/estimate_uncalibrated_relative_pose.cc:67-172) and
 * SampleConsensusEstimator::Estimate with InlierSupport (solvers/sample_consensus_estimator.h:246-344).  The calibrated
 * (five-point) branch is tmi_ba_estimate_calibrated_relative_poses further down.  Not provided: PROSAC, LMED and
 * exhaustive sampling, use_mle, use_Tdd_test, guided matching.
 * A one-shot call without a tmi_ba_problem.  Pair p owns the correspondences pair_offset[p] .. pair_offset[p + 1] - 1,
 * numbered 0..n-1; feature1 / feature2 [2 per correspondence] are CENTRED pixels: the principal point removed and NO
 * focal division, as NormalizeFeatures leaves them when a focal prior is missing (estimate_twoview_info.cc:82-85).
 * pair_error_threshold [num_pairs] is RansacParameters::error_thresh per pair, the SQUARED threshold in pixels^2
 * (:220-221: the product of the two resolution-scaled thresholds), computed by the caller.  pair_mask [num_pairs]
 * selects the pairs (NULL = all).  Per selected pair, in this order:
 *   1. n < 8 (the sampler refuses to initialise)                                                   -> status 1.
 *   2. The sample of iteration i.  samples_given != 0: the caller's samples[8 (max_iterations p + i) + k].  Otherwise
 *      deterministic in `seed` and stateless, as step 2 of tmi_ba_localize_views with 3 replaced by 8: word
 *      c = 8 (q 2^32 + i) + k (mod 2^64) of the splitmix64 stream from state `seed`, q = pair_stream[p] (EXTENSION; NULL:
 *      q = p), u = ((word >> 11) + 0.5) 2^-53, j_k = min(k + floor(u (n - k)), n - 1), then the eight swaps of a partial
 *      Fisher-Yates on the identity permutation, swap(a[k], a[j_k]) for k = 0..7; the sample is a[0..7].
 *      THE SAMPLE SEQUENCES ARE NOT THE REFERENCE'S (its RandomSampler carries its permutation along and draws from
 *      another generator).
 *   3. NormalizedEightPointFundamentalMatrix on the eight points (eight_point_fundamental_matrix.cc:54-113,
 *      pose/util.cc:82-115): per image the centroid (sums in sample order, / 8), rms = sqrt(sum((dx^2 + dy^2)) / 8),
 *      nf = sqrt(2) / rms, T = [nf 0 -nf cx; 0 nf -nf cy; 0 0 1]; the 8x9 rows
 *      (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1) of the normalised points; the kernel by elimination with FULL
 *      pivoting; the transpose (so that F(i, j) = f[3 i + j]); the nearest rank-2 matrix by a 3x3 SVD; F = T2^T F T1.
 *      What Eigen leaves open is fixed: the pivot is the entry of largest magnitude, ties go to the lowest (row,
 *      column); the rank counts the pivots with |pivot| > 8 DBL_EPSILON |largest pivot| (FullPivLU's default threshold
 *      for an 8x9 matrix) and a rank other than 8 gives NO MODEL; the kernel vector (back-substitution from 1 in the last
 *      permuted column, each sum in ascending column order) is normalised to unit length with its largest-magnitude entry
 *      (the first among equals) positive.  Every 3x3 SVD of this call is a one-sided Jacobi iteration on the columns:
 *      10 sweeps over the column pairs (0,1), (0,2), (1,2), a pair with a zero inner product skipped, then the columns
 *      sorted by descending squared norm with a stable network (a tie keeps the lower column first).  The rank-2 matrix
 *      is the sum of the two leading sigma_j u_j v_j^T.
 *   4. FocalLengthsFromFundamentalMatrix (fundamental_matrix_util.cc:57-133): the epipoles are the right null vectors of
 *      F and F^T, each formed as the cross product of two rows (of F, of F^T) with the largest squared norm among
 *      r0 x r1, r0 x r2, r1 x r2 (the first among equals), NOT normalised: the focal lengths depend on neither their
 *      length nor their sign.  epipole.x() == 0 for either gives no model.  The two in-plane rotations need no atan2, sin
 *      or cos: cos = e_x / r, sin = -e_y / r, r = sqrt(e_x^2 + e_y^2).  Then the factorised matrix and the two
 *      quotients in the reference's association.  A negative square gives no model; so does a NaN square (DEVIATION:
 *      the reference's `< 0` lets NaN through).
 *   5. EssentialMatrixFromFundamentalMatrix, E = diag(f2, f2, 1) F diag(f1, f1, 1), then GetBestPoseFromEssentialMatrix
 *      (essential_matrix_utils.cc:57-148) on the eight sampled correspondences divided by the two focal lengths: the
 *      SVD; with both determinant sign fixes applied the third columns of U and V are the cross products of their first
 *      two, and are formed so; rotation1 = U d V^T, rotation2 = U d^T V^T, translation = U.col(2).normalized(); the four
 *      candidates (R1, -R1^T t), (R1, R1^T t), (R2, -R2^T t), (R2, R2^T t) in the reference's order;
 *      IsTriangulatedPointInFrontOfCameras (triangulation.cc:216-232) per point; the FIRST candidate with the largest
 *      count wins (std::max_element).  Any count is accepted (:122-127).  (Which of the two SVD sign conventions a
 *      library picks permutes the four candidates; the winner differs only between candidates of equal count.)
 *   6. The cost of the ONE model of a sample: the correspondences (the eight sampled ones included) for which the
 *      cheirality test on the focal-normalised pair fails, or the SquaredSampsonDistance (pose/util.cc:56-68) of the
 *      CENTRED pixels under F is not below the threshold, or that distance is NaN.
 *   7. The replay is step 5 of tmi_ba_localize_views with a sample size of 8 and one model per sample: strict <;
 *      inlier_ratio < 8 / n skips the update of the bound; ComputeMaxIterations(8, ...) from a host-made table; a sample
 *      without a model counts as an iteration; THE RESULT DOES NOT DEPEND ON chunk_iterations (0: max(min_iterations,
 *      64)).
 *   8. Final: the inlier mask of the best model, num_inliers, confidence = 1 - (1 - (num_inliers / n)^8)^num_iterations
 *      (host); no model in any iteration -> status 2; otherwise status 0 and the model: fundamental_matrix [9]
 *      column-major as the reference stores it (as estimated: no scale is imposed), the focal lengths, the rotation as
 *      angle-axis (Ceres' RotationMatrixToAngleAxis, the routine tmi_ba_localize_views uses) and the position.
 * pair_status: -1 not selected, 0, 1, 2.  Every per-pair output [num_pairs] ([9 / 3 num_pairs]) may be NULL.
 * corr_inlier [pair_offset[num_pairs]] (optional): 1 for the inliers of the best model, 0 elsewhere.  hypothesis_cost
 * [num_selected * max_iterations] (optional, for tests; selected pairs in ascending index): the cost of every replayed
 * hypothesis, -1 for no model or not replayed.
 * ComputeMaxIterations and the confidence are evaluated on the host (log and pow of the C library); steps 3 to 6 use
 * + - * / and sqrt only and are never contracted into FMA.
 * TMI_BA_ERR_INVALID_ARGUMENT, before the device (options->device) is looked for: a null options or summary, a missing
 * array, a negative count, pair_offset that does not start at 0 or decreases, the CHECKs of the
 * SampleConsensusEstimator constructor (an error threshold of an attempted pair that is not positive, min_inlier_ratio
 * outside [0, 1], failure_probability outside (0, 1), max_iterations < min_iterations), max_iterations above 2^20, a
 * negative chunk_iterations, 2^31 - 1 correspondences or more, samples_given without samples, and a sample of an
 * attempted pair with a repeated or out-of-range index. */
typedef struct tmi_ba_two_view_ransac_options {
  double   failure_probability;  /* 0.01 (sample_consensus_estimator.h:57-65; EstimateTwoViewInfo sets
                                    1 - expected_ransac_confidence, estimate_twoview_info.h:69)                  */
  double   min_inlier_ratio;     /* 0                                                                          */
  int32_t  min_iterations;       /* 10   (EstimateTwoViewInfoOptions, estimate_twoview_info.h:70)              */
  int32_t  max_iterations;       /* 1000 (estimate_twoview_info.h:71)                                          */
  int32_t  chunk_iterations;     /* 0 = the engine's choice                                                    */
  int32_t  device;               /* -1 = the current device                                                    */
  uint64_t seed;                 /* 0                                                                          */
} tmi_ba_two_view_ransac_options;
void tmi_ba_two_view_ransac_options_init(tmi_ba_two_view_ransac_options* options);

typedef struct tmi_ba_two_view_ransac_summary {
  int32_t num_pairs;                    /* selected pairs                                   */
  int32_t num_estimated;                /* status 0                                         */
  int32_t num_too_few_correspondences;  /* status 1                                         */
  int32_t num_no_model;                 /* status 2                                         */
  int32_t num_chunks;                   /* chunks of iterations evaluated                   */
  int32_t reserved;
  int64_t total_iterations;             /* RANSAC iterations over the attempted pairs       */
  int64_t total_scores;                 /* correspondences times iterations replayed        */
  double  seconds;
  double  kernel_seconds;               /* the launches, first to last (the per-chunk read-back of the done flags
                                           included)                                        */
  double  hypothesis_seconds;           /* of kernel_seconds: the hypothesis launches,      */
  double  score_seconds;                /* the scoring launches                             */
  double  replay_seconds;               /* and the replay launches                          */
} tmi_ba_two_view_ransac_summary;

int32_t tmi_ba_estimate_uncalibrated_relative_poses(
    const tmi_ba_two_view_ransac_options* options, int32_t num_pairs, const int64_t* pair_offset,
    const double* feature1, const double* feature2, const double* pair_error_threshold, const uint8_t* pair_mask,
    const uint32_t* pair_stream, const int32_t* samples, int32_t samples_given, int8_t* pair_status,
    int32_t* pair_num_correspondences, int32_t* pair_num_inliers, int32_t* pair_num_iterations,
    int32_t* pair_best_iteration, double* pair_confidence, double* fundamental_matrix, double* focal_length1,
    double* focal_length2, double* rotation, double* position, uint8_t* corr_inlier, int32_t* hypothesis_cost,
    tmi_ba_two_view_ransac_summary* summary);

/* ---- batched EstimateRelativePose: five-point RANSAC for many calibrated view pairs ----------------------
 * reference: the CALIBRATED branch of EstimateTwoViewInfo (estimate_twoview_info.cc:127-200), taken whenever both views
 * carry a focal-length prior: EstimateRelativePose with RansacType::RANSAC (estimators/estimate_relative_pose.cc:59-144)
 * over FivePointRelativePose (pose/five_point_relative_pose.cc:212-299, the MINIMAL path) and
 * SampleConsensusEstimator::Estimate with InlierSupport.  Not provided: PROSAC, LMED and exhaustive sampling, use_mle
 * (MLESAC scoring), use_Tdd_test, the non-minimal (SVD) path of the solver.
 * A one-shot call shaped like tmi_ba_estimate_uncalibrated_relative_poses, whose options, summary, pair_offset,
 * pair_mask, pair_stream, samples / samples_given, integer outputs and corr_inlier it shares.  What differs:
 * feature1 / feature2 are NORMALISED coordinates, the principal point removed and the result divided by the focal
 * length, as NormalizeFeatures leaves them when both priors are set (estimate_twoview_info.cc:67-100);
 * pair_error_threshold is RansacParameters::error_thresh in those units (:160-162), computed by the caller; the model
 * is essential_matrix [9] (column-major, as the reference stores it; unit Frobenius norm), rotation [3] (angle-axis),
 * position [3]; pair_best_solution says which of a sample's models won; there are no focal-length outputs.  Per
 * selected pair, in this order:
 *   1. n < 5                                                                                       -> status 1.
 *   2. The sample of iteration i: step 2 of the uncalibrated call with 8 replaced by 5 (samples[5 (max_iterations p +
 *      i) + k]; word c = 5 (q 2^32 + i) + k; five swaps).
 *   3. FivePointRelativePose on the five points:
 *      a. The 5x9 rows (x2 x1, y2 x1, x1, x2 y1, y2 y1, y1, x2, y2, 1) (:227-236).  The kernel by elimination with FULL
 *         pivoting under the eight-point call's rules: the pivot is the entry of largest magnitude, strict >, ties to the
 *         lowest (row, column); the rank counts the pivots with |pivot| > 5 DBL_EPSILON |largest pivot|; a rank other
 *         than 5 gives NO MODEL.  The basis is FullPivLU::kernel()'s: one vector per free permuted column, that column
 *         1, the other free columns 0, back-substitution with each sum in ascending column order, NOT normalised.
 *      b. The 10x20 constraint matrix exactly as :65-206 expand it, their association order kept, no FMA contraction.
 *      c. C[:, :10] X = C[:, 10:] by elimination with full pivoting of the augmented matrix under the same rules, then
 *         back-substitution (ascending column order).  DEVIATION: a rank below 10 at 10 DBL_EPSILON gives NO MODEL (the
 *         reference solves whatever the rank).
 *      d. The action matrix (:271-279) and its REAL eigenvalues by one fixed algorithm: reduction to Hessenberg form
 *         by stabilised elementary similarity transformations (EISPACK elmhes: the pivot of column m - 1 is the entry
 *         of largest magnitude among rows m.., strict >, the first among equals), no balancing, then the Francis
 *         double-shift QR iteration to the real Schur form (EISPACK hqr: a subdiagonal entry e is negligible when
 *         |e| + s == s for s the sum of its two diagonal neighbours' magnitudes, or the matrix' norm where that is 0;
 *         exceptional shifts at sweeps 10 and 20).  A block that has not split after 30 sweeps gives NO MODEL; every
 *         loop has a fixed bound.  A root is real exactly where the Schur form leaves a 1x1 block, or a 2x2 block whose
 *         discriminant is >= 0 (the reference's imag() != 0 test).
 *      e. Per real eigenvalue, in ASCENDING order (equal ones in the order of their diagonal position; the reference's
 *         order is whatever Eigen returns, and matters only between models of equal cost): the null vector of
 *         A - lambda I by NINE steps of the same elimination, the tenth permuted entry set to 1.  DEVIATION: the rank
 *         test (10 DBL_EPSILON) covers the nine pivots; the tenth is the root's own rounding residual and is taken as
 *         zero.  Rank < 9 gives no model for that root.  The last four entries are the coordinates over the kernel
 *         basis; the 9-vector null_space x tail (:293-294) is scaled to unit norm with its largest-magnitude entry
 *         (the first among equals) positive.
 *   4. GetBestPoseFromEssentialMatrix on the five sampled correspondences: step 5 of the uncalibrated call (the same 3x3
 *      Jacobi SVD, candidates, cheirality vote, first of the largest) without focal division.  A model is kept only with
 *      at least 4 points in front (estimate_relative_pose.cc:94-104).  A sample yields 0 to 10 models in 10 slots, in
 *      the order of 3e.
 *   5. The cost of a model (:111-121): the correspondences for which the cheirality test fails, or the
 *      SquaredSampsonDistance under E is not below the threshold, or that distance is NaN.
 *   6. The replay is step 5 of tmi_ba_localize_views (many models per sample, ascending (iteration, slot), strict <)
 *      with a sample size of 5 and 10 slots; THE RESULT DOES NOT DEPEND ON chunk_iterations.
 *   7. Final: the inlier mask of the best model, confidence = 1 - (1 - (num_inliers / n)^5)^num_iterations (host); no
 *      model in any iteration -> status 2.
 * hypothesis_cost [num_selected * max_iterations * 10] (optional, for tests): -1 for an empty slot or not replayed.
 * Steps 3 to 5 use + - * / sqrt and fabs only and are never contracted into FMA.  The argument errors and their order
 * relative to the device check are those of the uncalibrated call, with 5 in place of 8. */
int32_t tmi_ba_estimate_calibrated_relative_poses(
    const tmi_ba_two_view_ransac_options* options, int32_t num_pairs, const int64_t* pair_offset,
    const double* feature1, const double* feature2, const double* pair_error_threshold, const uint8_t* pair_mask,
    const uint32_t* pair_stream, const int32_t* samples, int32_t samples_given, int8_t* pair_status,
    int32_t* pair_num_correspondences, int32_t* pair_num_inliers, int32_t* pair_num_iterations,
    int32_t* pair_best_iteration, int32_t* pair_best_solution, double* pair_confidence, double* essential_matrix,
    double* rotation, double* position, uint8_t* corr_inlier, int32_t* hypothesis_cost,
    tmi_ba_two_view_ransac_summary* summary);

/* ---- batched EstimateHomography: four-point RANSAC for many view pairs, inlier-count or MLESAC scoring ----
 * reference: the first step of TwoViewMatchGeometricVerification::VerifyMatches, CountHomographyInliers
 * (two_view_match_geometric_verification.cc:124, :326-363): EstimateHomography with RansacType::RANSAC
 * (estimators/estimate_homography.cc:54-117) over FourPointHomography (pose/four_point_homography.cc:72-101) and
 * SampleConsensusEstimator::Estimate (solvers/sample_consensus_estimator.h:246-344) with InlierSupport (use_mle == 0)
 * or MLEQualityMeasurement (use_mle != 0, solvers/mle_quality_measurement.h:58-71; the scoring CountHomographyInliers
 * passes on by default).  Not provided: PROSAC, LMED and exhaustive sampling, use_Tdd_test.
 * A one-shot call shaped like tmi_ba_estimate_uncalibrated_relative_poses, whose summary, pair_offset, pair_mask,
 * pair_stream, samples / samples_given, integer outputs and corr_inlier it shares.  What differs: feature1 / feature2
 * are in WHATEVER units the caller uses (pixels, centred pixels, normalised coordinates: H maps feature1 to feature2 in
 * them) and pair_error_threshold is RansacParameters::error_thresh in those units SQUARED; the model is homography [9];
 * the options are tmi_ba_homography_ransac_options, those of the sibling calls plus use_mle.  Per selected pair, in
 * this order:
 *   1. n < 4                                                                                       -> status 1.
 *   2. The sample of iteration i: step 2 of the uncalibrated call with 8 replaced by 4 (samples[4 (max_iterations p +
 *      i) + k]; word c = 4 (q 2^32 + i) + k; four swaps).  THE SAMPLE SEQUENCES ARE NOT THE REFERENCE'S.
 *   3. FourPointHomography on the four points.  Per image NormalizeImagePoints (pose/util.cc:82-115): the centroid (sums
 *      in sample order, / 4), rms = sqrt(sum((dx^2 + dy^2)) / 4), nf = sqrt(2) / rms, T = [nf 0 -nf cx; 0 nf -nf cy;
 *      0 0 1]; the normalised points hnormalized(T x) = (nf x + (-(nf cx)), nf y + (-(nf cy))).  The 8x9 rows of
 *      CreateActionConstraint (:55-64) in the reference's row and column order, for the normalised (a, b) of image 1 and
 *      (c, d) of image 2: row 2k = (0, 0, 0, -a, -b, -1, a d, b d, d), row 2k + 1 = (a, b, 1, 0, 0, 0, -(a c), -(b c),
 *      -c).  The null vector by elimination with FULL pivoting under the eight-point call's rules: the pivot is the
 *      entry of largest magnitude, strict >, ties to the lowest (row, column); the rank counts the pivots with
 *      |pivot| > 8 DBL_EPSILON |largest pivot|; back-substitution from 1 in the last permuted column, each sum in
 *      ascending column order; the vector is normalised to unit length with its largest-magnitude entry (the first among
 *      equals) positive.  H = T2^-1 M T1 with M(i, j) = null[3 i + j] and T2^-1 = [1/nf 0 cx; 0 1/nf cy; 0 0 1] in
 *      closed form: first G = M T1, then T2^-1 G.
 *      DEVIATIONS: the reference takes the null vector from a Jacobi SVD of A^T A (the same vector up to rounding and
 *      sign where the rank is 8); and a rank other than 8 gives NO MODEL -- three collinear points, a repeated point --
 *      as does a nf that is not finite (rms == 0, tested before the elimination), where the reference returns true for
 *      any sample and scores whatever vector the SVD leaves in a null space of dimension 2 or more.
 *   4. The residual of a correspondence (estimate_homography.cc:90-96, the asymmetric transfer error):
 *      p = H (x1, y1, 1), each row as (H0 x1 + H1 y1) + H2, r = (x2 - p0 / p2)^2 + (y2 - p1 / p2)^2.  Inlier iff
 *      r < threshold; a NaN r is an outlier.
 *   5. The cost of the ONE model of a sample.  use_mle == 0: the number of outliers, an integer.  use_mle != 0:
 *      MLEQualityMeasurement::ComputeCost, the double sum over the correspondences of (r < threshold ? r : threshold),
 *      and the integer inlier count of the same pass.  The sum has ONE FIXED SHAPE: lane l of 64 adds its
 *      correspondences l, l + 64, ... in ascending order starting from +0.0; the 64 partial sums are combined by the xor
 *      butterfly with offsets 32, 16, 8, 4, 2, 1 (lane l takes its own value + that of lane l ^ offset; every lane ends
 *      with the same value since addition is commutative).  Two runs give the same bytes.
 *   6. The replay is step 5 of tmi_ba_localize_views with a sample size of 4 and one model per sample: ascending
 *      iteration order, strict < on the cost (int from INT_MAX, or double from DBL_MAX); the bound is updated from the
 *      INLIER COUNT, which under MLE is not the cost, and only ever goes down; inlier_ratio < 4 / n skips the update;
 *      ComputeMaxIterations(4, ...) from a host-made table; a sample without a model counts as an iteration; THE RESULT
 *      DOES NOT DEPEND ON chunk_iterations (0: max(min_iterations, 64)).
 *   7. Final: the inlier mask of the best model, num_inliers, confidence = 1 - (1 - (num_inliers / n)^4)^num_iterations
 *      (host); no model in any iteration -> status 2; otherwise status 0 and homography [9] column-major as the
 *      reference stores an Eigen::Matrix3d, as estimated: no scale is imposed.
 * hypothesis_cost [num_selected * max_iterations] (optional, for tests): the integer cost of every replayed hypothesis,
 * or n - inliers under MLE; -1 for no model or not replayed.  hypothesis_cost_real [num_selected * max_iterations]
 * (optional, for tests): the MLE cost, NaN where hypothesis_cost is -1; passing it with use_mle == 0 is an argument
 * error.  Steps 3 to 5 use + - * / and sqrt only and are never contracted into FMA.  The argument errors and their order
 * relative to the device check are those of the uncalibrated call, with 4 in place of 8. */
typedef struct tmi_ba_homography_ransac_options {
  double   failure_probability;  /* 0.01                                                                       */
  double   min_inlier_ratio;     /* 0                                                                          */
  int32_t  min_iterations;       /* 10                                                                         */
  int32_t  max_iterations;       /* 1000                                                                       */
  int32_t  chunk_iterations;     /* 0 = the engine's choice                                                    */
  int32_t  device;               /* -1 = the current device                                                    */
  uint64_t seed;                 /* 0                                                                          */
  int32_t  use_mle;              /* 0 = inlier-count scoring; nonzero = MLESAC (RansacParameters::use_mle)     */
  int32_t  reserved;             /* 0                                                                          */
} tmi_ba_homography_ransac_options;
void tmi_ba_homography_ransac_options_init(tmi_ba_homography_ransac_options* options);

int32_t tmi_ba_estimate_homographies(
    const tmi_ba_homography_ransac_options* options, int32_t num_pairs, const int64_t* pair_offset,
    const double* feature1, const double* feature2, const double* pair_error_threshold, const uint8_t* pair_mask,
    const uint32_t* pair_stream, const int32_t* samples, int32_t samples_given, int8_t* pair_status,
    int32_t* pair_num_correspondences, int32_t* pair_num_inliers, int32_t* pair_num_iterations,
    int32_t* pair_best_iteration, double* pair_confidence, double* homography, uint8_t* corr_inlier,
    int32_t* hypothesis_cost, double* hypothesis_cost_real, tmi_ba_two_view_ransac_summary* summary);

/* ---- batched EstimateAbsolutePoseWithKnownOrientation: two-point position RANSAC for many views -----------
 * reference: EstimateAbsolutePoseWithKnownOrientation with RansacType::RANSAC
 * (estimators/estimate_absolute_pose_with_known_orientation.cc:54-150; what the assume_known_orientation branch of
 * LocalizeViewToReconstruction, localize_view_to_reconstruction.cc:160-185, calls -- that branch itself stays refused)
 * over PositionFromTwoRays (pose/position_from_two_rays.cc:56-83) and SampleConsensusEstimator::Estimate
 * (solvers/sample_consensus_estimator.h:246-344) with InlierSupport (use_mle == 0) or MLEQualityMeasurement
 * (use_mle != 0, solvers/mle_quality_measurement.h:58-71).  Not provided: PROSAC, LMED and exhaustive sampling,
 * use_Tdd_test.
 * A one-shot call shaped like tmi_ba_estimate_homographies, whose options, summary (an item is a view here),
 * item_offset / item_mask / item_stream, samples / samples_given, integer outputs, corr_inlier and the two
 * hypothesis-cost arrays it shares.  feature [2 n] are NORMALISED image coordinates (principal point removed, divided
 * by the focal length), NOT yet rotated; world_point [3 n]; item_orientation [3 per item] the view's angle-axis
 * (world to camera); item_error_threshold is RansacParameters::error_thresh, squared normalised units.  The estimator
 * has no min_num_inliers.  Per selected item, in this order:
 *   1. n < 2                                                                                       -> status 1.
 *   2. RotateCorrespondences (:54-73), one device thread per correspondence: R = ceres::AngleAxisToRotationMatrix of
 *      the item's orientation (the engine's restatement, first-order branch at theta^2 <= DBL_EPSILON; it calls sin and
 *      cos, the only such functions in the call), ray_i = (R(0,i) u + R(1,i) v) + R(2,i), the rotated feature
 *      (ray_0 / ray_2, ray_1 / ray_2).  rotated_feature [2 n] (optional): what this step left, 0 for items not attempted;
 *      every later step is a function of it that uses + - * / and sqrt only, never contracted into FMA.
 *   3. The sample of iteration i: step 2 of the homography call with 4 replaced by 2 (samples[2 (max_iterations p + i)
 *      + k]; word c = 2 (q 2^32 + i) + k; two swaps).  THE SAMPLE SEQUENCES ARE NOT THE REFERENCE'S.
 *   4. PositionFromTwoRays on the two (rotated feature (u_k, v_k), point (X_k, Y_k, Z_k)): the least-squares solution
 *      of the 4x3 system with rows [1 0 -u_k], [0 1 -v_k] and right side b = (X_1 - u_1 Z_1, Y_1 - v_1 Z_1,
 *      X_2 - u_2 Z_2, Y_2 - v_2 Z_2) through its normal equations in closed form: du = u_1 - u_2, dv = v_1 - v_2,
 *      q = du du + dv dv, c_z = -((du (b_0 - b_2) + dv (b_1 - b_3)) / q), c_x = ((b_0 + u_1 c_z) + (b_2 + u_2 c_z)) / 2,
 *      c_y = ((b_1 + v_1 c_z) + (b_3 + v_2 c_z)) / 2.  RANK RULE: the pivots of the normal equations are 2, 2 and q / 2;
 *      with n22 = (u_1^2 + v_1^2) + (u_2^2 + v_2^2) their largest diagonal entry is max(2, n22); rank 3 iff
 *      q / 2 > (3 DBL_EPSILON)^2 max(2, n22), else NO MODEL.  (The reference: ColPivHouseholderQR::rank() != 3 at
 *      3 DBL_EPSILON on R's diagonal, the square roots of such pivots; the two rules differ by a bounded factor at a
 *      boundary only two rotated features equal to 1e-15 reach.)
 *   5. The residual (:106-113): d = X - c, r = (d_0 / d_2 - u)^2 + (d_1 / d_2 - v)^2.  There is NO cheirality test, as in
 *      the reference.  Inlier iff r < threshold; a NaN r is an outlier.
 *   6. The cost, the replay and the chunking: steps 5 and 6 of the homography call with a sample size of 2 (the fixed
 *      64-lane shape of the MLE sum included; inlier_ratio < 2 / n skips the update of the bound).
 *   7. Final: the inlier mask of the best model, num_inliers, confidence = 1 - (1 - (num_inliers / n)^2)^num_iterations
 *      (host); no model in any iteration -> status 2; otherwise status 0 and position [3].
 * The argument errors and their order relative to the device check are those of the homography call, with 2 in place
 * of 4; item_orientation is a required array whenever num_items > 0. */
int32_t tmi_ba_estimate_positions_known_orientation(
    const tmi_ba_homography_ransac_options* options, int32_t num_items, const int64_t* item_offset,
    const double* feature, const double* world_point, const double* item_orientation,
    const double* item_error_threshold, const uint8_t* item_mask, const uint32_t* item_stream, const int32_t* samples,
    int32_t samples_given, int8_t* item_status, int32_t* item_num_correspondences, int32_t* item_num_inliers,
    int32_t* item_num_iterations, int32_t* item_best_iteration, double* item_confidence, double* position,
    uint8_t* corr_inlier, int32_t* hypothesis_cost, double* hypothesis_cost_real, double* rotated_feature,
    tmi_ba_two_view_ransac_summary* summary);

/* ---- batched EstimateRelativePoseWithKnownOrientation: two-point baseline RANSAC for many view pairs ------
 * reference: EstimateRelativePoseWithKnownOrientation with RansacType::RANSAC
 * (estimators/estimate_relative_pose_with_known_orientation.cc:19-82) over RelativePoseFromTwoPointsWithKnownRotation
 * (pose/relative_pose_from_two_points_with_known_rotation.cc:51-88), either scoring.  Not provided: PROSAC, LMED and
 * exhaustive sampling, use_Tdd_test.
 * The call above with two features per correspondence and no world point.  The reference takes correspondences the
 * caller has already rotated, rf = hnormalize(R^t K^-1 [u v 1]^t) (relative_pose_from_two_points_with_known_rotation.h:
 * 43-47); here feature1 / feature2 [2 n] are normalised and NOT rotated, and step 2 rotates feature1 by
 * pair_orientation1 and feature2 by pair_orientation2 ([3 per pair] each, the two views' angle-axes; all zero: the
 * features pass through bit for bit).  rotated_feature1 / rotated_feature2 [2 n] (optional) as above.  What differs:
 *   1. n < 2                                                                                       -> status 1.
 *   4. The rows e_k = (-y1 + y2, -x2 + x1, y1 x2 - x1 y2) of the two sampled correspondences (:65-74).  RANK RULE: two
 *      steps of elimination with FULL pivoting under the sibling calls' rules (the pivot is the entry of largest
 *      magnitude, strict >, ties to the lowest (row, column)); rank 2 iff both pivots are > 0 and
 *      min(p0, p1) > 2 DBL_EPSILON max(p0, p1) -- FullPivLU's rule for a 2x3 matrix -- else NO MODEL
 *      (dimensionOfKernel() != 1).  The null vector is c = e_0 x e_1, each entry a b - c d as written, divided by
 *      sqrt((c_0^2 + c_1^2) + c_2^2); a norm that is 0 or not finite gives no model.  SIGN RULE: the sign of e_0 x e_1
 *      as computed, rows in sample order, NO flip; the reference's sign is whatever FullPivLU::kernel() leaves, and
 *      only the direction up to sign is the estimate (position [3] is +-(c2 - c1) / |c2 - c1| in the rotated frame).
 *   5. The residual (:52-58): SquaredSampsonDistance (pose/util.cc:56-68) of (feature1, feature2) under
 *      F = CrossProductMatrix(-t) = [0 t2 -t1; -t2 0 t0; t1 -t0 0], the zero entries left out of the sums:
 *      l = (t2 y1 - t1, t0 - t2 x1, t1 x1 - t0 y1), num = (x2 l0 + y2 l1) + l2, g = (t1 - y2 t2, x2 t2 - t0),
 *      r = num^2 / (((g0^2 + g1^2) + l0^2) + l1^2).  The reference's Error has NO behind-camera rule and never returns
 *      DBL_MAX, so neither does this.
 *   7. confidence with the exponent 2; position [3] has unit length. */
int32_t tmi_ba_estimate_relative_positions_known_orientation(
    const tmi_ba_homography_ransac_options* options, int32_t num_pairs, const int64_t* pair_offset,
    const double* feature1, const double* feature2, const double* pair_orientation1, const double* pair_orientation2,
    const double* pair_error_threshold, const uint8_t* pair_mask, const uint32_t* pair_stream, const int32_t* samples,
    int32_t samples_given, int8_t* pair_status, int32_t* pair_num_correspondences, int32_t* pair_num_inliers,
    int32_t* pair_num_iterations, int32_t* pair_best_iteration, double* pair_confidence, double* position,
    uint8_t* corr_inlier, int32_t* hypothesis_cost, double* hypothesis_cost_real, double* rotated_feature1,
    double* rotated_feature2, tmi_ba_two_view_ransac_summary* summary);

/* Test hook: FNV-1a checksums of the static structure arrays resident in HBM -- built in HBM by
 * sort / scan kernels (one rank, no shared intrinsics blocks; TMI_BA_HOST_SETUP=1 disables) or on
 * host threads otherwise.  out[0] = 1 when the device built it; the other slots are documented at
 * the definition (engine.hip).  The two builders must agree array for array. */
int32_t tmi_ba_solver_structure_checksums(tmi_ba_solver* solver, uint64_t out[24]);

/* Which kernels a handle will run -- decided at create from the problem's shape and size (bench.py reports the
 * bytes of the kernel that ran instead of re-deriving the engine's rules):
 *   out[0] the one-sweep matrix-free product is built (mf_chunks.h)        out[1] position columns formed from Jp
 *   out[2] matrix-free LM iterations build the camera side without camera-major records (direct_diag.h)
 *   out[3] schur_mode auto chooses the operator per LM iteration           out[4] S is never formed (implicit)
 *   out[5] PCG length up to which the matrix-free operator is taken (auto)
 *   out[6] the handle holds clusters for CLUSTER_JACOBI (0: such a request keeps the SCHUR_JACOBI blocks, and
 *          tmi_ba_summary.effective_preconditioner_type says so)
 *   out[7] bit 0: the planes of the handle's last linearisation are COMPACT: on the all-PINHOLE / default-mask /
 *          TRIVIAL-loss problem with unit aspect ratio and zero skew the camera block is formed from the point block, the
 *          normalised image point, the track and the view instead of stored (TMI_BA_COMPACT_PLANES=0 switches it off)
 *          bit 1: the handle may linearise the candidate of a trial step speculatively instead of taking its trial cost
 *          (TMI_BA_SPECULATIVE_LINEARIZE=0 switches it off)
 *          bit 2: back-substitution can take y_p and the model cost change from the per-track sums the PCG solve's
 *          matrix-free products left instead of sweeping the observations again (one rank, the one-sweep product, no
 *          shared intrinsics blocks; TMI_BA_BACKSUB_FROM_PRODUCTS=0 switches it off)
 *          bits 8..: LM iterations of the handle's last solve that took that path                                       */
int32_t tmi_ba_solver_operator_info(tmi_ba_solver* solver, int32_t out[8]);

/* Host-only: statistics of the static structure the engine would build for
 * rank `rank` of `world` (no GPU needed).  Used by the CPU tests of the track
 * sharding: out[0] tracks owned, out[1] observations owned, out[2] reduced
 * blocks, out[3] block dimension D, out[4] upper off-diagonal blocks of S,
 * out[5] BSR blocks, out[6] observation pairs owned, out[7] checksum of the
 * (rank independent) block list, out[8] slices, out[9] padded observations,
 * out[10] checksum of the owned caller observation indices, out[11] sum over
 * owned pairs of a (slot independent) pair key.  Returns a tmi_ba_status. */
int32_t tmi_ba_structure_stats(const tmi_ba_problem* problem, int32_t rank, int32_t world,
                               int64_t out[12]);
/* The same for the dealing a handle actually uses: slices go to the ranks longest-work-first, and "work" is Schur
 * pairs + 5 x observations where the handle forms S (forms_S = 1: schur_mode explicit, exact solvers -- what
 * tmi_ba_structure_stats reports) but the track's observations where the operator is matrix-free (forms_S = 0: the
 * default of a solve on several ranks, schur_mode auto / implicit). */
int32_t tmi_ba_structure_stats_for(const tmi_ba_problem* problem, int32_t rank, int32_t world, int32_t forms_S,
                                   int64_t out[12]);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* THEIA_MI355_BA_H_ */
