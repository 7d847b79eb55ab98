/*
 * mantis.h — C-ABI of the MI355X-native mantis3 hot path (libmantis_amd.so).
 *
 * Drop-in boundary for the reference's per-frame callback and service:
 *   void quadDetection(const sensor_msgs::ImageConstPtr&,
 *                      const sensor_msgs::CameraInfoConstPtr&)   src/mantis3.cpp:68-135
 *   srv/mantisService.srv:1-13 (Image[] image, CameraInfo[] camera_info,
 *        Vector3 delta_pos, Quaternion delta_quat -> Pose pose, float64 weight,
 *        int32 num_particles)                                    (server: src/mantis_server.cpp:23-30)
 * Plain C types only (no ROS/OpenCV/torch types). Every entry point returns a
 * mantis_status; mantis_last_error() describes the last failure on a context.
 * The library never calls exit()/abort() (the reference does: RPP.cpp:450-453).
 *
 * Ownership: input buffers are borrowed for the call only; host inputs are
 * staged through pinned memory. The context owns all device memory and its
 * HIP stream. Threading: one context per host thread; calls on one context are
 * serialized (matching the reference's single ros::spin thread,
 * src/mantis3.cpp:155). State carried across frames (the reference's globals
 * `cv::RNG rng(1)` Mantis3Params.h:87 and the map) lives in the context.
 */
#ifndef MANTIS_H
#define MANTIS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MANTIS_ABI_VERSION 5

typedef enum mantis_status {
  MANTIS_OK = 0,
  MANTIS_ERR_ARG = 1,       /* bad argument (null pointer, size, channel count) */
  MANTIS_ERR_DEVICE = 2,    /* HIP runtime / kernel failure, or no GPU */
  MANTIS_ERR_OOM = 3,       /* device or pinned allocation failed */
  MANTIS_ERR_CAPACITY = 4,  /* a fixed-capacity workspace overflowed (see last_error) */
  MANTIS_ERR_STATE = 5,     /* map not set, comm not initialised, ... */
  MANTIS_ERR_COMM = 6       /* RCCL failure */
} mantis_status;

/* Per-frame outcome (reference early returns / gates, src/mantis3.cpp:82-132). */
typedef enum mantis_reason {
  MANTIS_PUBLISHED = 0,      /* yaw gap > MINIMUM_YAW_DIFFERENCE, pose published (PosePub.h:16) */
  MANTIS_NO_QUADS = 1,       /* "no quadrilaterlals detected!" early return (mantis3.cpp:82-84) */
  MANTIS_NO_HYPS = 2,        /* empty cluster (mantis3.cpp:94-97) */
  MANTIS_YAW_AMBIGUOUS = 3,  /* pose computed but gate not met: not published */
  MANTIS_NO_YAW = 4          /* every yaw set scored DBL_MAX (reference UB) */
} mantis_reason;

typedef struct mantis_config {
  int32_t struct_size;          /* sizeof(mantis_config) */
  int32_t device;               /* HIP device ordinal */
  int32_t max_cams;             /* camera-frames per mantis_process_batch call */
  int32_t max_width, max_height; /* width <= 8190, height <= 65533, width x height < 2^25 (else MANTIS_ERR_ARG) */
  uint64_t rng_seed;            /* cv::RNG seed, 1 in the reference (Mantis3Params.h:87) */
  int32_t canny_low;            /* ~canny_hysteresis, 50 (Mantis3Params.h:162); high = 3x */
  int32_t polygon_epsilon;      /* ~polygon_epsilon, 10 (:164) */
  double search_radius_multiplier; /* ~neighborhood_search_radius_multiplier, 0.1 (:166) */
  double grid_spacing;          /* ~grid_spacing, 0.32 (:167) */
  int32_t particles, iterations;/* 50, 10 (PoseAdjustment.h:29) */
  int32_t gn_enable;            /* 0 = reference-parity mode (no GN refinement) */
  int32_t gn_iterations;        /* rig GN iterations (0..10) */
  int32_t max_quads;            /* per-frame quad capacity: 256 (0 = default); other values are rejected */
  int32_t max_contour_points;   /* per-frame contour point pool (default 262144) */
  int32_t quad_gn_iterations;   /* per-quad GN after RPP (4 corners <-> model square), 0 = off (parity) */
  int32_t rig_weighting;        /* rig fusion: 0 = lowest-error published camera (default);
                                   1 = legacy MonteCarlo weighting (see mantis_get_rig_weights) */
} mantis_config;

typedef struct mantis_image {   /* sensor_msgs/Image (bgr8) + sensor_msgs/CameraInfo */
  int32_t width, height;
  int32_t step_bytes;           /* row stride, >= 3*width */
  int32_t mem_kind;             /* 0 = host pointer, 1 = device pointer (already in HBM) */
  const uint8_t* bgr;
  double K[9];                  /* CameraInfo.K, row-major; rounded to float as get3x3FromVector does */
  double D[4];                  /* fisheye k1..k4 (CameraInfo.D) */
  double T_base_cam[16];        /* camera pose in the rig/base frame (row-major 4x4); identity for 1 cam */
  int64_t stamp_ns;
  const char* frame_id;
} mantis_image;

typedef struct mantis_motion {  /* mantisService delta_pos / delta_quat ("applied to each particle") */
  double delta_pos[3];
  double delta_quat_xyzw[4];
} mantis_motion;

typedef struct mantis_cam_result {
  int32_t status;
  int32_t reason;               /* mantis_reason */
  int32_t publish;
  int32_t n_quads;              /* after removeDuplicateQuads */
  int32_t n_hyps;               /* after clustering (C) */
  int32_t n_scored;             /* hypotheses scored (fast + slow) */
  double position[3];           /* published camera position (w2c origin, PosePub.h:33-45) */
  double orientation_xyzw[4];
  double covariance[36];        /* diag(error / 600) (PosePub.h:47-56) */
  double error;                 /* hyp.error of the published hypothesis (COLOR error) */
  double min_yaw_diff;
  double pf_error;              /* fast error of the particle-filter optimum */
  double c2w[12];               /* published hypothesis, world->camera R (row-major) | t */
} mantis_cam_result;

typedef struct mantis_result {  /* one rig pose (mantisService response + diagnostics) */
  int32_t status;
  int32_t publish;
  int32_t n_cams_published;
  int32_t num_particles;        /* srv num_particles: hypotheses scored over the rig */
  double position[3];           /* srv pose (base frame in world) */
  double orientation_xyzw[4];
  double covariance[36];
  double weight;                /* srv weight: error of the chosen camera hypothesis */
  double min_yaw_diff;
  int32_t n_quads;
  int32_t gn_iterations;
  double gn_cost;               /* final GN cost (0 when GN disabled) */
  uint64_t rng_state_after;
} mantis_result;

/* ---------------------------------------------------------------- context */
void mantis_default_config(mantis_config* cfg);
mantis_status mantis_create(const mantis_config* cfg, void** out_ctx);
mantis_status mantis_destroy(void* ctx);
const char* mantis_last_error(void* ctx);
int32_t mantis_abi_version(void);

/* whiteMap / redMap / greenMap (params/map.yaml, parsed as Mantis3Params.h:125-152) */
mantis_status mantis_set_map(void* ctx, const double* white_xyz, int32_t nw, const double* red_xyz, int32_t nr,
                             const double* green_xyz, int32_t ng);
/* parseCoordinatesFromString (Mantis3Params.h:125-152); returns the row count, writes up to max_pts */
int32_t mantis_parse_coordinates(const char* s, double* xyz, int32_t max_pts);

/* cv::RNG state (checkpoint / resume of the cross-frame particle-filter stream) */
mantis_status mantis_rng_get(void* ctx, uint64_t* state);
mantis_status mantis_rng_set(void* ctx, uint64_t state);

/* ------------------------------------------------------------ hot path */
/* One rig pose from n_cams synchronized cameras (n_cams = 1 is exactly the
 * reference callback quadDetection, src/mantis3.cpp:68-135). cam_out may be
 * NULL; otherwise it receives n_cams per-camera results. motion (nullable) is
 * the mantisService delta_pos / delta_quat ("applied to each particle before
 * reevaluating", srv/mantisService.srv:4-8): the context keeps the last
 * published rig pose as the service's particle; with a motion and that prior,
 * T_prior * Transform(delta_quat, delta_pos) joins the rig candidates and all
 * are re-evaluated with the legacy weighting (mantis_get_rig_weights, last
 * candidate slot). Without a prior, or with |delta_quat|^2 < 0.5 (an unset
 * message), the call is the reference callback. */
mantis_status mantis_process(void* ctx, const mantis_image* cams, int32_t n_cams, const mantis_motion* motion,
                             mantis_result* out, mantis_cam_result* cam_out);
/* the motion prior (last published rig pose, T_w_b row-major 4x4): set (NULL clears) / get */
mantis_status mantis_set_prior_pose(void* ctx, const double* T_w_b);
mantis_status mantis_get_prior_pose(void* ctx, double* T_w_b, int32_t* has_prior);
/* n_rigs rigs of cams_per_rig cameras in one batched pass (throughput path):
 * cams[r * cams_per_rig + c]; frames are processed (and draw RNG) in that order. */
mantis_status mantis_process_batch(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                   mantis_result* out, mantis_cam_result* cam_out);

/* Camera-sharded rig (BASELINE config 4: 8 cameras, one per GPU; SURVEY §8 e).
 * Every rank of the communicator (mantis_comm_init) calls this with the same
 * n_rigs / cams_per_rig and its own cameras: local_cams[r * n_local + j] is
 * camera cam_index[j] (ascending) of rig r; each camera belongs to exactly one
 * rank and n_local <= ceil(cams_per_rig / nranks). Exchanges (RCCL over xGMI):
 * one ncclAllGather of the frames' particle-filter flags, so every frame
 * draws the cv::RNG stream at the offset a sequential run over the rig's
 * cameras in rig-major order would (Mantis3Params.h:87, PoseAdjustment.h:15-16);
 * one ncclAllGather of the camera results for the rig fusion; with gn_enable one
 * ncclAllReduce of every rig's J^T J / J^T r accumulators per Gauss-Newton
 * iteration (each rank then solves the same 6x6 system). The multi-camera seam of
 * the reference is the base->camera extrinsic chain of
 * include/legacy/mantis/MonteCarlo.cpp:250-271. Every rank returns the same
 * out[n_rigs]; cam_out (nullable) receives all n_rigs * cams_per_rig camera
 * results in global order. With one rank this equals mantis_process_batch. */
mantis_status mantis_process_rig_sharded(void* ctx, const mantis_image* local_cams, int32_t n_rigs, int32_t n_local,
                                         const int32_t* cam_index, int32_t cams_per_rig, mantis_result* out,
                                         mantis_cam_result* cam_out);

/* Stage entry of the sharded call's cross-rank RNG bookkeeping (device
 * kernel k_gauss_offsets_global, for parity tests): `pairs` = the gathered
 * (global frame index, reaches-PF flag) pairs of every rank (npairs pairs,
 * padding slots (-1, 0)); each of the n_local frames with global index gidx[i]
 * gets offsets[i] = per_frame x (frames before it in global order that reach
 * the particle filter), i.e. where a sequential run over all cameras draws its
 * cv::RNG gaussians (Mantis3Params.h:87, PoseAdjustment.h:15-16); *total = the
 * gaussians drawn by all n_global frames. Host rule: mantis_amd/csrc/mk_shard.h. */
mantis_status mantis_shard_gauss_offsets(void* ctx, const int32_t* pairs, int32_t npairs, int32_t n_global,
                                         const int32_t* gidx, int32_t n_local, int32_t per_frame, int32_t* offsets,
                                         int32_t* total);

/* Rig Gauss-Newton record of rig `rig` of the last batch (cfg.gn_enable):
 * the fused pose the correspondences were formed with, the refined pose, the
 * cost before / after, and this rank's correspondences as rows of
 * [local camera index, u, v, X, Y, Z] (normalized undistorted point, world point). */
typedef struct mantis_rig_gn_info {
  double T_init[16];
  double T_final[16];
  double cost0, cost;
  int32_t valid, iterations, n_obs, n_obs_local;
} mantis_rig_gn_info;
mantis_status mantis_get_rig_gn(void* ctx, int32_t rig, mantis_rig_gn_info* info, double* obs, int32_t cap);

/* Rig weighting (cfg.rig_weighting = 1): the legacy particle
 * weight MonteCarlo::computeWeight / computeCameraError
 * (include/legacy/mantis/MonteCarlo.cpp:183-241) made to work with every
 * camera of the rig (the reference's "TODO make work with both cameras",
 * :250-271). Candidate k = the base pose implied by published camera k
 * (T_w_b = T_w_c inv(T_base_cam)); camera c scores it with
 * computeCameraError: every landmark projected into c (no z test, the float
 * pixel strictly inside (0, cols) x (0, rows), cvRound), the squared BGR
 * distance to its set's colour (white / red / green targets, mantis3's
 * palette Mantis3Params.h:40-42), error = sum / n, or 1e17 / n when n < 10.
 * The legacy undistortImage + pinhole projection is replaced by mantis3's
 * fisheye projection of the original frame (distortPixel, Mantis3Types.h:
 * 125-136). Weight = mean over the rig's cameras; the lowest weight wins
 * (first on ties) and is the rig's srv weight. Camera-sharded rigs sum the
 * per-camera (error sum, count) slots with one ncclAllReduce (exact integers).
 * Record of rig `rig` of the last batch, K = C + 1 candidate slots (C =
 * cams_per_rig; slot C = the mantisService motion prediction, see
 * mantis_process): weights[K] (DBL_MAX = not a candidate), c2w[K x C x 12]
 * (world->camera of candidate k in camera c, this rank's cameras; nullable),
 * sums[K x C x 2] (sum, count; nullable), chosen = winning slot or -1. */
mantis_status mantis_get_rig_weights(void* ctx, int32_t rig, double* weights, double* c2w, double* sums,
                                     int32_t* chosen);
/* Shape of the last batch's weighting record: rigs and C (cameras per rig), so
 * a caller sizes the buffers of mantis_get_rig_weights (K = C + 1 slots). */
mantis_status mantis_get_rig_weights_info(void* ctx, int32_t* n_rigs, int32_t* cams_per_rig);

/* Markov yaw filter (include/mantis3/Markov.{h,cpp}, MarkovModel,
 * included but unused upstream): n_filters 360-bin yaw distributions in the
 * context's HBM (one per camera stream or rig). w2c_R: hypothesis poses' w2c
 * bases (row-major 3x3, one per filter / hypothesis); yaw bin = getRPY yaw in
 * degrees wrapped to [0, 360). active (nullable): filter f is updated iff
 * active[f] != 0. Results are bit-identical to oracle/o_markov.cpp. */
/* MarkovModel(Hypothesis) (Markov.cpp:15-27): one-hot at the yaw bin, blurred (stddev 3) */
mantis_status mantis_markov_init(void* ctx, int32_t n_filters, const double* w2c_R);
/* senseFusion(Hypothesis) (:164-201): multiply by the measurement (stddev 3.5), normalize */
mantis_status mantis_markov_sense(void* ctx, const double* w2c_R, const int32_t* active);
/* convolve(dTheta, dt) (:227-258): shift by (int)dTheta*180/pi bins (dTheta truncated to whole
 * radians first, as the reference), blur with stddev dt * 11.5 / 90 */
mantis_status mantis_markov_convolve(void* ctx, const double* dtheta, const double* dt, const int32_t* active);
/* updateHypothesis (:207-222) with filter `filter`: error[i] = error[i] * 1 / p[bin(w2c_R[i])] */
mantis_status mantis_markov_weight(void* ctx, int32_t filter, const double* w2c_R, int32_t n, double* error);
/* planes (n_filters x 360, nullable); yaw = getYaw (:265-275: p[argmax] * pi / 180, the reference's
 * return value; nullable); argmax = first maximum bin (nullable) */
mantis_status mantis_markov_get(void* ctx, double* planes, double* yaw, int32_t* argmax);

/* ------------------------------------------- stage entry points (parity) */
/* gray -> GaussianBlur 3x3 -> Canny(50,150) (QuadDetection.h:209-212); out W*H bytes 0/255 */
mantis_status mantis_canny(void* ctx, const mantis_image* img, uint8_t* canny_out);
/* cv::Canny's hysteresis alone (the stack walk of QuadDetection.h:212 / HypothesisEvaluation.h:327's
 * Canny): cls W*H bytes, 0 = no candidate, 1 = weak candidate (NMS passed, mag > low), 2 = strong
 * (mag > high); out W*H bytes 0/255 = the candidates 8-connected to a strong pixel. Any other
 * class byte (e.g. a 0/255 plane) returns MANTIS_ERR_ARG */
mantis_status mantis_hysteresis(void* ctx, const uint8_t* cls, int32_t width, int32_t height, uint8_t* edges_out);
/* detector binary (dilate x2, erode x1, QuadDetection.h:213-214) and the
 * cleanImageByEdge mask (HypothesisEvaluation.h:319-386); either output may be NULL */
mantis_status mantis_masks(void* ctx, const mantis_image* img, uint8_t* det_out, uint8_t* mask_out);
/* detectQuadrilaterals (QuadDetection.h:203-287): int corners x0,y0..x3,y3 per quad,
 * after removeDuplicateQuads, in reference order */
mantis_status mantis_detect_quads(void* ctx, const mantis_image* img, int32_t* corners, int32_t max_quads,
                                  int32_t* n_quads);
/* evaluateHypotheses (HypothesisEvaluation.h:31-41, 71-158) fast=1 (1 px, all landmarks vs WHITE)
 * or evaluateHypothesisCOLOR (:89-105, 160-266) fast=0 (10x10 window, green vs GREEN).
 * c2w: n x 12 doubles (world->camera R row-major | t). mask: W*H bytes (nonzero = keep) or NULL
 * (score img as given). err: error per hypothesis (DBL_MAX if no projection), nproj: counts. */
mantis_status mantis_score_hypotheses(void* ctx, const mantis_image* img, const uint8_t* mask, const double* c2w,
                                      int32_t n, int32_t fast, double* err, int32_t* nproj);
/* RPP::Rpp on n 4-point problems (RPP.cpp:13-64): img_pts n x 4 x 2 normalized, obj_pts n x 4 x 3.
 * R n x 9, t n x 3, errs n x 2 (obj_err, img_err), rpp_status n (1 ok, 0 2nd-pose search failed,
 * -1 rotation check failed = the reference's exit(1)). */
mantis_status mantis_rpp_batch(void* ctx, const double* img_pts, const double* obj_pts, int32_t n, double* R,
                               double* t, double* errs, int32_t* rpp_status);
/* RPP::Rpp(model, iprts, ...) (RPP.h:92-93, RPP.cpp:13-64) on n problems of n_points points each,
 * 4 <= n_points <= 12 (the reference accepts any count; demo.cpp:17-38 solves 10): img_pts
 * n x n_points x 2 normalized (the homogeneous row is 1, as demo.cpp's Mat::ones), obj_pts
 * n x n_points x 3. Outputs as mantis_rpp_batch plus iterations (n, nullable: the reference's
 * `iterations` out-parameter). One device lane per problem; mantis_rpp_batch is the throughput
 * entry for 4-point problems (same arithmetic, bit-identical results). */
mantis_status mantis_rpp_solve(void* ctx, const double* img_pts, const double* obj_pts, int32_t n_points,
                               int32_t n, double* R, double* t, double* errs, int32_t* rpp_status,
                               int32_t* iterations);

/* Per-quad Gauss-Newton after RPP (new stage; legacy analogue
 * cv::solvePnP ITERATIVE, include/legacy/mantis2/PoseEstimator.h:91-153): n
 * problems of 4 normalized image points img_pts (n x 4 x 2) and model points
 * obj_pts (n x 4 x 3); R (n x 9), t (n x 3) hold the starting pose (model ->
 * camera, e.g. mantis_rpp_batch's) and receive the refined one. Up to
 * `iterations` steps minimizing the normalized reprojection error; a step is
 * kept only if the cost decreases. steps (n, nullable) = steps kept, costs
 * (n x 2, nullable) = r^T r before / after. The same refinement runs inside
 * the pipeline after RPP when cfg.quad_gn_iterations > 0. */
mantis_status mantis_quad_gn(void* ctx, const double* img_pts, const double* obj_pts, int32_t n, double* R,
                             double* t, int32_t iterations, int32_t* steps, double* costs);

/* Dense scoring with an argmin (BASELINE config 5: 81 shifts x 4 yaws x 50
 * perturbations = 16,200 hypotheses, SURVEY §8 d/e): the fast evaluator
 * (evaluateHypotheses, HypothesisEvaluation.h:31-41, 71-158) on n hypotheses,
 * then the lowest error with the first index on ties (the strict "<" the
 * reference's best-1 choice keeps). Hypothesis k of this call has global index
 * index_base + k. With use_comm (after mantis_comm_init) every rank passes its
 * shard and one ncclAllGather of (err, index) pairs gives all ranks the global
 * winner. best_idx = -1 when no hypothesis was scored (n == 0 on every rank);
 * hypotheses that all see nothing tie at DBL_MAX and give the first index. */
mantis_status mantis_score_argmin(void* ctx, const mantis_image* img, const uint8_t* mask, const double* c2w,
                                  int32_t n, int64_t index_base, int32_t use_comm, double* best_err,
                                  int64_t* best_idx);
/* The same with device-resident inputs: mask_dev (W*H bytes, or NULL) and c2w_dev
 * (n x 12 doubles) are device pointers on the context's GPU (mantis_device_alloc
 * or any allocation of that device), read in place -- no staging copy -- for
 * callers whose hypotheses are produced on the device or reused across calls. */
mantis_status mantis_score_argmin_dev(void* ctx, const mantis_image* img, const uint8_t* mask_dev,
                                      const double* c2w_dev, int32_t n, int64_t index_base, int32_t use_comm,
                                      double* best_err, int64_t* best_idx);
/* The cross-shard rule on its own (host only): pairs = nranks x (err, global index). */
mantis_status mantis_argmin_pick(const double* pairs, int32_t nranks, double* best_err, int64_t* best_idx);

/* mantis_score_argmin_dev over n_frames frames in one call (BASELINE config 5
 * batched): frame f's n_hyps[f] hypotheses (device c2w_dev[f], n x 12) scored
 * against its cleaned mask (device masks_dev[f], nullable array / entries)
 * in one launch, one argmin per frame, and with use_comm one ncclAllGather of
 * every frame's (err, global index) pair per rank; best_err / best_idx get
 * n_frames entries (global index = index_base[f] + local index). */
mantis_status mantis_score_argmin_batch(void* ctx, const mantis_image* imgs, int32_t n_frames,
                                        const uint8_t* const* masks_dev, const double* const* c2w_dev,
                                        const int32_t* n_hyps, const int64_t* index_base, int32_t use_comm,
                                        double* best_err, int64_t* best_idx);

/* ----------------------------------------- Gauss–Newton rig refinement (new) */
/* One GN step over m camera observations: for camera c, corr_c normalized image points u (2)
 * matched to world points X (3). Accumulates J^T J (21 upper-tri), J^T r (6), cost (1) into
 * acc28 for the base pose T_w_b (4x4 row-major) with right-perturbation exp(delta).
 * obs: rows of [cam_index, u_x, u_y, X, Y, Z]; T_base_cam: 16 doubles per camera. */
mantis_status mantis_gn_accumulate(void* ctx, const double* T_w_b, const double* T_base_cam, int32_t n_cams,
                                   const double* obs, int32_t n_obs, double* acc28);
/* Solve (JtJ + lambda I) delta = -Jtr from acc28 and update T_w_b in place. */
mantis_status mantis_gn_solve(const double* acc28, double lambda, double* T_w_b, double* delta6);

/* ------------------------------------------------- multi-GPU (RCCL, xGMI) */
/* 128-byte ncclUniqueId; rank 0 creates it, the caller broadcasts it. */
mantis_status mantis_comm_unique_id(void* id128);
mantis_status mantis_comm_init(void* ctx, const void* id128, int32_t nranks, int32_t rank);
/* the communicator's size and this context's rank (MANTIS_ERR_STATE without one) */
mantis_status mantis_comm_info(void* ctx, int32_t* nranks, int32_t* rank);
/* Camera-sharded rig: this rank contributes its cameras; the 28-double GN
 * accumulators are summed with one ncclAllReduce per iteration. */
mantis_status mantis_gn_allreduce(void* ctx, double* acc28);

/* ------------------------------------------------------------- tools */
/* Synthetic fisheye grid frames rendered in HBM (bench inputs). cams: n x mantis_synth_cam;
 * out_dev: device buffer n x H x W x 3 (stride 3W). */
typedef struct mantis_synth_cam {
  double fx, fy, cx, cy;
  double k[4];
  double R_wc[9];
  double pos[3];
  int32_t w, h;
  int32_t pad[2];
} mantis_synth_cam;
mantis_status mantis_synth_render(void* ctx, const mantis_synth_cam* cams, int32_t n, const uint64_t* seeds,
                                  uint8_t* out_dev);
/* Device buffers owned by the context (for device-resident benchmark inputs). */
mantis_status mantis_device_alloc(void* ctx, size_t bytes, void** dev_ptr);
mantis_status mantis_device_free(void* ctx, void* dev_ptr);
mantis_status mantis_memcpy_h2d(void* ctx, void* dst_dev, const void* src_host, size_t bytes);
mantis_status mantis_memcpy_d2h(void* ctx, void* dst_host, const void* src_dev, size_t bytes);
mantis_status mantis_synchronize(void* ctx);
/* Per-kernel timing of the last call (HIP events on the context stream), in ms. */
int32_t mantis_kernel_times(void* ctx, const char** names, float* ms, int32_t max);
/* Enable stage timing events (1) or not (0). */
mantis_status mantis_set_profiling(void* ctx, int32_t on);

/* ------------------------------------------------------- diagnostics */
/* Stage-by-stage record of camera-frame `frame` of the last batch (quads,
 * hypotheses, PF/shift/yaw errors); layout = oracle/oracle.h orc_frame_debug. */
size_t mantis_frame_debug_size(void);
mantis_status mantis_get_frame_debug(void* ctx, int32_t frame, void* out, size_t bytes);
/* The border-following output of camera-frame `frame` of the last batch
 * (findContours(RETR_CCOMP, CHAIN_APPROX_SIMPLE), QuadDetection.h:216, in the
 * library's border order): per border its point count and hole flag, and all
 * points (x, y pairs, image coordinates) border after border. Fails with
 * MANTIS_ERR_CAPACITY when max_borders / max_points are too small. */
mantis_status mantis_get_contours(void* ctx, int32_t frame, int32_t* counts, int32_t* holes, int32_t max_borders,
                                  int32_t* points, int32_t max_points, int32_t* n_borders);
/* Work counters of camera-frame `frame` of the last batch: borders, contour
 * points, raw/kept quads, generated/clustered hypotheses, PF flag, gaussian
 * offset, overflow flags, then 7 contour-kernel phase ends (10 ns ticks).
 * Returns the number of int32 written (<= max), -1 on a bad argument. */
int32_t mantis_frame_counters(void* ctx, int32_t frame, int32_t* out, int32_t max);
/* Batches of at most this many frames take the latency kernels (tile Canny, segmented
 * morphology walker, LDS border walks, 1024-thread contour blocks), larger ones the
 * throughput kernels; both give identical results (CUs / 4 by default,
 * MANTIS_FC_SMALL_FRAMES). No reference counterpart: a tuning query. */
int32_t mantis_small_batch_frames(void* ctx);

/* ------------------------------------------------- rig tracking (ABI 3) */
/* Joint multi-camera particle filter from a pose prior: the reference's
 * particle filter (optimizeHypothesisWithParticleFilter, PoseAdjustment.h:13-60)
 * seeded from a predicted rig pose instead of from detection, its particles
 * rig base poses T_w_b, each scored on every camera of the rig with the sums
 * pooled (the mantisService's "delta applied to each particle before
 * reevaluating", srv/mantisService.srv:4-8; MonteCarlo.cpp:250's "TODO make
 * work with both cameras"). Only the image stages up to the cleanImageByEdge
 * mask run: no contours, RPP, hypothesis generation, shifts or yaw sets.
 *
 * Pooled error of a base pose T: for each camera c the fast WHITE evaluator
 * (HypothesisEvaluation.h:107-158, 218-227) on c's cleaned frame with
 * c2w_c = inverse(T * T_base_cam_c) gives exact integers (sum_c, n_c);
 * E = (double)sum(sum_c) / ((double)sum(n_c) * 1.1), DBL_MAX when sum(n_c) = 0.
 * cur = the prediction, iter_err[0] = seed_error = E(cur). Iteration k = 1 ..
 * iterations: particle j = cur * rand_j, rand_j = Transform(setRPY(roll,
 * pitch, yaw), (x, y, z)) from six gaussians of the context's cv::RNG drawn
 * yaw, pitch, roll (x sigma_rot), z, y, x (x sigma_t), applied on the right
 * in the base frame; the first strict minimum (argmin by (E, j)) replaces cur
 * only when it is < the current error; iter_pick[k-1] = that j or -1,
 * iter_err[k] = the current error afterwards. Every rig draws particles x
 * iterations x 6 gaussians, rigs in order, tracked or not. */
typedef struct mantis_track_params {
  int32_t struct_size;      /* sizeof(mantis_track_params) */
  int32_t particles;        /* 1..96 */
  int32_t iterations;       /* 0..10; 0 = score the prediction only */
  double sigma_rot, sigma_t; /* >= 0 (sigma_rot <= 1e6); 0 is legal (particles equal the current pose) */
  int32_t min_projections;  /* gate: pooled in-frame landmark count, default 10 (MonteCarlo.cpp:220) */
  int32_t record;           /* 1 = keep the per-iteration record (mantis_get_track_record) */
  double max_error;         /* gate: <= 0 means none */
} mantis_track_params;
/* 50 / 10 / 0.03 / 0.01 (cfg.particles / cfg.iterations when ctx is given and they fit), 10, 0, 0 */
void mantis_default_track_params(void* ctx /* nullable */, mantis_track_params* p);

typedef struct mantis_track_result {
  int32_t status, tracked, n_proj, n_scored; /* n_proj = sum(n_c) at T_w_b; n_scored = 1 + particles x iterations */
  double T_w_b[16];         /* refined base pose, row-major */
  double error, seed_error; /* pooled fast error after / of the prediction */
  double iter_err[11];      /* [0] = seed, [k] = current error after iteration k (k > iterations: = error) */
  int32_t iter_pick[10];    /* [k-1] = particle accepted in iteration k, -1 = none (also past `iterations`) */
  uint64_t rng_state_after; /* cv::RNG state after this rig's draws */
} mantis_track_result;
/* sizeof(mantis_track_params), sizeof(mantis_track_result) (host only) */
void mantis_track_sizes(int32_t* params_bytes, int32_t* result_bytes);

/* n_rigs rigs of cams_per_rig cameras (cams[r * cams_per_rig + c], one frame
 * size), rig r refined from T_w_b_pred[r] (n_rigs x 16, row-major).
 * tracked = error != DBL_MAX && n_proj >= min_projections && (max_error <= 0
 * || error <= max_error). MANTIS_ERR_ARG (nothing launched): no map, n_rigs x
 * cams_per_rig > max_cams, cams_per_rig > 8, particles x cams_per_rig > 512,
 * frames of different sizes, a parameter outside its range. */
mantis_status mantis_track_batch(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                 const double* T_w_b_pred, const mantis_track_params* p, mantis_track_result* out);
/* One rig from the context's prior (mantis_set_prior_pose / the last published
 * pose): prediction = prior * Transform(delta_quat, delta_pos), the prior
 * itself when motion is NULL or unset (|q|^2 < 0.5). MANTIS_ERR_STATE without
 * a prior. Tracked: the prior becomes T_w_b and out is a published rig
 * (publish = 1, pose from T_w_b, covariance = diag(error / 600), weight =
 * error, num_particles = n_scored). Not tracked: publish = 0, the prior stays;
 * the caller falls back to mantis_process. tout (nullable) gets the details. */
mantis_status mantis_track(void* ctx, const mantis_image* cams, int32_t n_cams, const mantis_motion* motion,
                           const mantis_track_params* p, mantis_result* out, mantis_track_result* tout);
/* Record of rig `rig` of the last track call made with record = 1: iteration
 * k = 1 .. iterations, or -1 = the seed (one "particle", the prediction).
 * T_w_b: P x 16, c2w: P x C x 12 (world -> camera R row-major | t), sums /
 * counts: P x C integer error sums and landmark counts; each nullable.
 * *n_particles = P of that pass (1 for the seed). */
mantis_status mantis_get_track_record(void* ctx, int32_t rig, int32_t iteration, double* T_w_b, double* c2w,
                                      int64_t* sums, int32_t* counts, int32_t* n_particles);

/* ---------------------------------------- Monte Carlo localization (ABI 4) */
/* A persistent, weighted, resampled population of rig base poses T_w_b in the
 * context's HBM: the filter the mantisService contract implies (delta_pos /
 * delta_quat "applied to each particle before reevaluating", weight,
 * num_particles; srv/mantisService.srv) and the legacy MonteCarlo.cpp never
 * became. One filter per context. One step (mantis_mcl_step), exactly:
 *  1. Draws: N x 6 gaussians of the context's cv::RNG, particle-major, each
 *     particle's six drawn yaw, pitch, roll, z, y, x (as mantis_track), then
 *     one raw 32-bit output U (state = (uint32)state * 4164903690 + (state >>
 *     32), U = (uint32)state): on every step, whatever the sigmas and outcome.
 *  2. Predict: T_j <- T_j * Delta * rand_j(sigma_rot, sigma_t), Delta =
 *     Transform(delta_quat, delta_pos), the identity when motion is NULL or
 *     unset (|q|^2 < 0.5); everything applied on the right.
 *  3. Score: the image stages up to the cleanImageByEdge mask, then for every
 *     (particle, camera) the exact integers (sum, n) of the fast WHITE
 *     evaluator with c2w = inverse(T_j * T_base_cam_c); E_j = the pooled error
 *     of mantis_track. Particle j is valid iff E_j != DBL_MAX and n_j >=
 *     min_projections.
 *  4. Weights in fixed point: L_j <- L_j - E_j / tau (valid), -inf (others);
 *     Lmax = max L_j; q_j = (uint64)floor(exp(L_j - Lmax) * 2^40) (0 for L_j =
 *     -inf); S = sum q_j and the inclusive sums c_j are exact integers, the same
 *     in any reduction order. No particle with a finite L_j: the step is lost
 *     (lost = 1, out->publish = 0, the particles keep their predicted poses
 *     and their previous log-weights, nothing is resampled, the context's
 *     prior pose is untouched).
 *  5. Estimate: w_j = q_j / S; position sum w_j t_j; rotation = the normalised
 *     w-weighted sum of the particles' quaternions (Matrix3x3::getRotation),
 *     each with the sign that has a non-negative dot with particle best's --
 *     best's own basis if that sum's norm is < 1e-12 or only one particle has
 *     q > 0; covariance = sum w_j xi_j xi_j^T, xi_j = [t_j - t ; log(R^T R_j)],
 *     order x, y, z, rot-x, rot-y, rot-z row-major (ROS PoseWithCovariance;
 *     translation in the world frame, rotation a right perturbation);
 *     ess = S^2 / sum q_j^2; best = the heaviest particle, the first on ties.
 *  6. Resample iff ess < resample_frac * N: systematic, ancestor a_i = the
 *     first j with c_j N 2^32 > (U + i 2^32) S in exact integer arithmetic,
 *     clamped to the last particle with q > 0; new particle i = old particle
 *     a_i, every L = 0. Otherwise the poses and the L_j stay.
 *  7. Output (not lost): publish = 1, the pose and the 6 x 6 covariance of the
 *     estimate, weight = best_error, num_particles = N; the context's prior
 *     pose becomes the estimate (mantis_track / mantis_process with a motion
 *     can take over).
 * Default tau: the median over 32 four-camera 720p synthetic rigs of
 * E(truth moved 2 cm and 1 degree) - E(truth), so that a particle that far
 * off keeps about 1/e of the best weight. Measured on an MI355X with
 * tools/mcl_latency.py: median 63478 (quartiles 59181 / 69064, range 46559 ..
 * 76800; E(truth) itself has the median 19658). DESIGN.md 4b. */
#define MANTIS_MCL_TAU_DEFAULT 63478.0
typedef struct mantis_mcl_params {
  int32_t struct_size;        /* sizeof(mantis_mcl_params) */
  int32_t n_particles;        /* 1..4096 */
  double sigma_rot, sigma_t;  /* per-step diffusion, >= 0 (sigma_rot <= 1e6), finite */
  double tau;                 /* > 0, finite: log-likelihood = -E / tau */
  double resample_frac;       /* 0..2: resample when ess < resample_frac * N (0 = never, 2 = always) */
  int32_t min_projections;    /* a particle with fewer pooled in-frame landmarks gets weight 0 */
  int32_t record;             /* 1 = keep the last step's record (mantis_mcl_get_record) */
} mantis_mcl_params;
/* 256 / 0.03 / 0.01 / MANTIS_MCL_TAU_DEFAULT / 0.5 / 10 / 0 */
void mantis_default_mcl_params(mantis_mcl_params* p);

typedef struct mantis_mcl_result {
  int32_t status, lost, resampled, n_particles;
  int32_t n_valid, best;      /* particles with q > 0; the heaviest one (first on ties), -1 when lost */
  double ess, best_error;     /* S^2 / sum q^2; E of particle best (0 / DBL_MAX when lost) */
  double T_w_b[16];           /* the estimate, row-major (zeros when lost) */
  double covariance[36];
  uint64_t weight_sum;        /* S */
  uint32_t U, pad;            /* the resampling draw */
  uint64_t rng_state_after;
} mantis_mcl_result;
/* sizeof(mantis_mcl_params), sizeof(mantis_mcl_result) (host only) */
void mantis_mcl_sizes(int32_t* params_bytes, int32_t* result_bytes);

/* Start the filter: particle j = T_w_b_mean * rand_j(sigma_rot0, sigma_t0)
 * from N x 6 gaussians drawn as in a step (and nothing else), every L = 0.
 * MANTIS_ERR_ARG (the filter and the RNG stay as they were): a parameter
 * outside its range, a null pointer, a NaN. */
mantis_status mantis_mcl_init(void* ctx, const double* T_w_b_mean, double sigma_rot0, double sigma_t0,
                              const mantis_mcl_params* p);
/* The same from given poses (N x 16, row-major); draws nothing. */
mantis_status mantis_mcl_init_particles(void* ctx, const double* T_w_b, const mantis_mcl_params* p);
/* One step on n_cams synchronized cameras of one size (1..8, <= max_cams).
 * MANTIS_ERR_STATE before an init; MANTIS_ERR_ARG (nothing launched, nothing
 * drawn): no map, frames of different sizes, n_cams out of range, a NaN
 * motion. mout is nullable. */
mantis_status mantis_mcl_step(void* ctx, const mantis_image* cams, int32_t n_cams, const mantis_motion* motion,
                              mantis_result* out, mantis_mcl_result* mout);
/* The particles as they stand: T_w_b (N x 16) and log_w (N) nullable, *n = N. */
mantis_status mantis_mcl_get(void* ctx, double* T_w_b, double* log_w, int32_t* n);
/* The last step's record (params.record = 1), each pointer nullable: the
 * predicted T_w_b (N x 16), c2w (N x C x 12, world -> camera R row-major | t),
 * sums / counts (N x C), L before and after the step (N each), q and cum (N
 * uint64; zeros when lost), ancestors (N int32, -1 each when not resampled),
 * *n_particles = N, *n_cams = C. */
mantis_status mantis_mcl_get_record(void* ctx, double* T_w_b_pred, double* c2w, int64_t* sums, int32_t* counts,
                                    double* L_before, double* L_after, uint64_t* q, uint64_t* cum,
                                    int32_t* ancestors, int32_t* n_particles, int32_t* n_cams);
/* Drop the filter (the next step needs an init); draws nothing. */
mantis_status mantis_mcl_reset(void* ctx);

/* ------------------------------- Monte Carlo localization: the modes (ABI 5) */
/* The floor grid is periodic: until a coloured border comes into view the
 * posterior has one mode per lattice cell and heading, and the step's mean of
 * a set that spans several of them is not a pose. These calls seed the set
 * over the lattice, read it back as one estimate per cell, and commit to one.
 * None of them draws beyond what is said, and mantis_mcl_step is unchanged.
 *  Key of a pose T against the anchor A (g = config.grid_spacing): ix =
 *     (int)floor((T.t[0] - A.t[0]) / g + 0.5), iy likewise from t[1]; the yaw
 *     quadrant k from the base x-axes projected on the world's xy plane, h =
 *     (T.R[0][0], T.R[1][0]), a = A's: c = h . a, s = a0 h1 - a1 h0; |c| >=
 *     |s|: k = c >= 0 ? 0 : 2; otherwise k = s > 0 ? 1 : 3 (c = s = 0: 0).
 *     |ix|, |iy| <= 7 is in range: bin = ((iy + 7) 15 + (ix + 7)) 4 + k, 900
 *     bins; everything else is the one bin "outside", counted, never a mode.
 *  Anchor: particle `best` of the last step's predicted set.
 *  Per bin, over the particles with q_j > 0: W = sum q_j (uint64, exact in any
 *     order), n = their number, the heaviest particle (the first on ties).
 *  Mode order: the non-empty in-range bins by W descending, then bin ascending.
 *  Per mode, the step's estimate (5. above) restricted to the bin with w_j =
 *     q_j / W: moments about the bin's heaviest particle, that particle's own
 *     basis when n = 1, covariance about the mean; share = W / S; best_error =
 *     the pooled error of the bin's heaviest particle. */
typedef struct mantis_mcl_mode {
  int32_t ix, iy, yaw_quadrant; /* the key against the anchor */
  int32_t n, best, pad;         /* particles with q > 0 in the bin; the heaviest (-1: an empty record) */
  uint64_t weight;              /* W */
  double share, best_error;     /* W / S; E of particle best (0 / DBL_MAX in an empty record) */
  double T_w_b[16];             /* the bin's estimate, row-major (zeros in an empty record) */
  double covariance[36];
} mantis_mcl_mode;
/* The tag shares the call's name: write `struct mantis_mcl_modes`. */
struct mantis_mcl_modes {
  int32_t status, n_modes;      /* records filled: min(max_modes, n_cells) */
  int32_t n_cells, n_outside;   /* non-empty in-range bins; particles with q > 0 outside */
  uint64_t weight_sum, outside_weight; /* S; the part of it outside */
  double anchor_T_w_b[16];      /* row-major (zeros after a lost step) */
  mantis_mcl_mode mode[8];      /* in mode order; empty records from n_modes on */
};
/* sizeof(mantis_mcl_mode), sizeof(struct mantis_mcl_modes) (host only) */
void mantis_mcl_modes_sizes(int32_t* mode_bytes, int32_t* modes_bytes);

/* mantis_mcl_init over a (2 cells_x + 1) x (2 cells_y + 1) lattice of the
 * grid: the same N x 6 gaussians in the same order, particle j = T_w_b_mean *
 * rand_j as there, then t[0] + (double)ix * g and t[1] + (double)iy * g with
 * site s = j % n_sites, ix = s % (2 cells_x + 1) - cells_x, iy = s / (2
 * cells_x + 1) - cells_y. cells 0, 0 is mantis_mcl_init. Yaw alternatives are
 * not seeded (mantis_mcl_init_particles takes any set; the keys still tell
 * them apart). MANTIS_ERR_ARG as mantis_mcl_init, and: cells_x / cells_y
 * outside 0..7, n_particles < n_sites. */
mantis_status mantis_mcl_init_lattice(void* ctx, const double* T_w_b_mean, double sigma_rot0, double sigma_t0,
                                      int32_t cells_x, int32_t cells_y, const mantis_mcl_params* p);
/* The modes of the last step, from what it left in HBM (predicted poses, q,
 * sums and counts; record = 0 or 1): the first min(max_modes, n_cells) of the
 * mode order, max_modes 1..8. One launch, one copy back. After a lost step:
 * MANTIS_OK, n_modes = 0. MANTIS_ERR_STATE: no step since the last init or
 * reset. MANTIS_ERR_ARG: max_modes out of range, out NULL. Changes nothing in
 * the filter. */
mantis_status mantis_mcl_modes(void* ctx, int32_t max_modes, struct mantis_mcl_modes* out);
/* Commit to mode mode_index of the last mantis_mcl_modes call: every particle
 * of the current set (the resampled one if the step resampled) whose key
 * against the same anchor differs from the mode's gets L = -inf, the others
 * keep their L, and the context's prior pose becomes the mode's T_w_b. A
 * dropped particle stays dropped until a resampling replaces it: the next
 * step's ess falls and its resampling repopulates the set from the kept mode.
 * MANTIS_ERR_STATE: no mantis_mcl_modes call since the last step, or no
 * particle of the current set lies in the mode (a light mode may leave no
 * offspring in a resampling) -- then nothing changes. MANTIS_ERR_ARG:
 * mode_index not below n_modes. */
mantis_status mantis_mcl_select_mode(void* ctx, int32_t mode_index);

/* ---------------- Monte Carlo localization: the colour evidence (additions) */
/* The step's scorer is the fast WHITE evaluator, which cannot tell one cell of
 * the floor grid from the next. These calls let the set also weigh the green
 * border with the reference's slow COLOR evaluator (computePointError(...,
 * GREEN, fast = false), HypothesisEvaluation.h:233-266) on the raw frames.
 * They only add: with enable = 0 a step is the step above, bit for bit, and
 * the ABI version stays 5 (look the entry points up by name, or call
 * mantis_mcl_color_sizes).
 *  Colour sums of (particle j, camera c), c2w as in 3. above: every green
 *     landmark in map order, projected exactly in FP64, is scored iff z > 0 and
 *     inFrame(u, v); its window sum is the integer sum over ox, oy in -5..4 of
 *     (b - 50)^2 + (g - 255)^2 + (r - 85)^2 at linear offset cvRound(v + oy) W +
 *     cvRound(u + ox) of the raw BGR frame, an offset outside [0, W H) reading
 *     0, 0, 0. csum (int64) = the sum of the window sums, cn (int32) = the
 *     number of scored landmarks.
 *  Pooled colour error: Ec_j = (double)sum_c csum / ((double)sum_c cn * 100.0 *
 *     1.1), defined when sum_c cn >= min_color_projections; DBL_MAX otherwise.
 *  Charge: charge_j = Ec_j / color_tau when defined, color_miss / color_tau
 *     otherwise (a particle must not win by seeing no green at all).
 *  enable = 2: step 4. becomes L_j <- (L_j - E_j / tau) - charge_j for the
 *     valid particles, in that operation order; validity (by the WHITE counts
 *     alone) and everything after are unchanged, a lost step leaves L as it was.
 *  enable = 1: the sums, Ec and the charge are computed and kept, the weights
 *     are those of enable = 0.
 *  A map without green landmarks: every cn = 0, every Ec = DBL_MAX, every
 *     charge = color_miss / color_tau.
 * One more launch per step (5 instead of 4) while enable >= 1.
 * Defaults, measured with the CPU oracle over the 32 four-camera 720p
 * synthetic rigs of tools/mcl_latency.py (tools/mcl_color_defaults.py), among
 * the rigs with >= 10 green landmarks in view at the truth (all 32; 120 .. 148
 * of the 4 x 37 are in view): color_miss = the median Ec(truth) = 15447.3
 * (quartiles 14224.9 / 16948.3, range 11028.7 .. 18415.8); color_tau = the
 * median of Ec(truth moved one cell, 0.32 m, along world y) - Ec(truth) =
 * 33379.0 (quartiles 30605.8 / 36813.5, range 25760.0 .. 44890.9; positive on
 * every rig), so that a particle one cell off keeps about 1/e per step from
 * colour alone. DESIGN.md 4d. */
#define MANTIS_MCL_COLOR_MISS_DEFAULT 15447.3
#define MANTIS_MCL_COLOR_TAU_DEFAULT 33379.0
typedef struct mantis_mcl_color_params {
  int32_t struct_size;            /* sizeof(mantis_mcl_color_params) */
  int32_t enable;                 /* 0 = off; 1 = score and record only; 2 = score and fold into L */
  double color_tau;               /* > 0, finite */
  double color_miss;              /* >= 0, finite: Ec of a particle with too few green landmarks in view */
  int32_t min_color_projections;  /* >= 1 */
  int32_t pad;
} mantis_mcl_color_params;
/* 0 / MANTIS_MCL_COLOR_TAU_DEFAULT / MANTIS_MCL_COLOR_MISS_DEFAULT / 10 */
void mantis_default_mcl_color_params(mantis_mcl_color_params* p);
/* sizeof(mantis_mcl_color_params) (host only) */
void mantis_mcl_color_sizes(int32_t* params_bytes);
/* Legal at any time after mantis_create; persists across inits and resets,
 * applies from the next step, draws nothing. MANTIS_ERR_ARG (nothing changes):
 * a null pointer, struct_size, enable outside 0..2, color_tau not finite and
 * > 0, color_miss not finite and >= 0, min_color_projections < 1. */
mantis_status mantis_mcl_set_color(void* ctx, const mantis_mcl_color_params* p);
/* The last step's colour record, whatever params.record says, each pointer
 * nullable: csums / ccounts (N x C) of the predicted set, Ec (N, DBL_MAX
 * where undefined) and charge (N); *n_particles = N, *n_cams = C. The arrays
 * stay in HBM until asked for. MANTIS_ERR_STATE: no step since the last init
 * or reset, or that step ran with enable = 0. */
mantis_status mantis_mcl_get_color_record(void* ctx, int64_t* csums, int32_t* ccounts, double* Ec, double* charge,
                                          int32_t* n_particles, int32_t* n_cams);
/* For each mode of the last mantis_mcl_modes call, Ec and sum_c cn of the
 * mode's heaviest particle (mode[i].best), 8 entries each; DBL_MAX / 0 in
 * empty records. Reads back, launches nothing, changes nothing. With enable =
 * 1 a server chooses the mode by colour and commits with
 * mantis_mcl_select_mode. MANTIS_ERR_STATE: no mantis_mcl_modes call since
 * the last step, or that step ran with enable = 0. MANTIS_ERR_ARG: a null
 * pointer. */
mantis_status mantis_mcl_modes_color(void* ctx, double* color_error /*8*/, int32_t* color_n /*8*/);

/* ---- Line refinement: Gauss-Newton on the grid lines from a pose prior ----
 * A continuous refinement that needs no detection and reads the raw BGR
 * frames only (no image stage runs, nothing is drawn: the cv::RNG state is
 * untouched). MANTIS_ABI_VERSION stays 5: callers find these entries by name
 * and check the struct sizes through mantis_refine_sizes.
 *
 * Landmarks: all n = nw + nr + ng in map order; target colour by set, BGR:
 * WHITE (255, 255, 255), RED (50, 85, 255), GREEN (50, 255, 85).
 * Line flags (host, cached until the next mantis_set_map or another
 * landmark_pitch): bit 0 of landmark i is set iff some landmark j != i lies at
 * X_i +- (pitch, 0, 0), every coordinate agreeing within 1e-6; bit 1 the same
 * along y. A candidate has flags exactly 1 (tangent e = x) or exactly 2
 * (e = y); intersections (and the map's duplicated intersection landmarks)
 * have both and are never used. Candidates are numbered in ascending landmark
 * order (n_cand of them).
 *
 * One observation of (base pose T, camera c, candidate i), R_cb / t_cb =
 * inverse(T_base_cam_c):
 *  1. q = R_wb^T (X - t_wb), p = R_cb q + t_cb; p_z <= 0: code 1.
 *  2. iz = 1 / p_z, m0 = (p_x iz, p_y iz), Jpi = [[iz, 0, -p_x iz^2], [0, iz, -p_y iz^2]].
 *  3. t = Jpi (R_cb R_wb^T e); |t| < 1e-12: code 2. th = t / |t|, nh = (-th_y, th_x).
 *  4. samples k = -R .. R, step s = 1 / fx (the float-rounded K): (u_k, v_k) =
 *     distort(m0 + (k s) nh, 1), x_k = cvRound(u_k), y_k = cvRound(v_k); a
 *     sample that is not finite or has x_k outside [0, W) or y_k outside
 *     [0, H): code 3.
 *  5. at pixel (x_k, y_k) of the raw frame: d2_k = sum_ch (pix - target)^2,
 *     w_k = max(0, white_thresh - d2_k), int32.
 *  6. w_-R > 0 or w_R > 0: code 4 (the line must lie strictly inside the window).
 *  7. Sw = sum w_k, Skw = sum k w_k (exact int32); Sw < min_weight: code 5.
 *  8. else code 0: d = ((double)Skw / (double)Sw) s, residual r = -d,
 *     h = (nh^T Jpi) R_cb, row J = [-h | h [q]x].
 * The first failing test decides the code; a row with a non-zero code is seven
 * zeros (and Sw = Skw = 0 for codes 1..3). Row slot = c n_cand + candidate;
 * no compaction (zero rows add exact zeros).
 *
 * Pass k = 0 .. I - 1 at pose T_k: the observations; acc28 = the upper
 * triangle of J^T J (21), J^T r (6), r^T r (1); n_obs[k] = the code-0 rows,
 * rms[k] = sqrt(r^T r / n_obs) (normalized image units; x fx ~ pixels; 0 when
 * n_obs = 0); n_obs < min_obs: status STARVED (1), stop; (J^T J + lambda I)
 * not positive definite: status SINGULAR (2), stop; else T_k+1 = T_k
 * Exp(delta[k]) (right perturbation, translation then rotation vector).
 * After the loop one more observation pass at the last pose gives the final
 * n_obs, rms and acc28 (I + 1 passes; I = 0 returns the pose bit for bit).
 * iterations_run = the steps taken; the final figures are n_obs /
 * rms[iterations_run] (a rig that stopped keeps those of the pass that stopped
 * it: same pose, same observations). Entries past it are 0.
 * refined = status OK && final n_obs >= min_obs && (max_rms <= 0 || final rms
 * <= max_rms). covariance (host): sigma^2 = r^T r / (n_obs - 6), Cov_delta =
 * sigma^2 (J^T J)^-1 by Cholesky, translation block turned to the world frame
 * (B Cov B^T, B = diag(R_wb, I)); order x, y, z, rot-x, rot-y, rot-z,
 * row-major. A non-PD J^T J or n_obs <= 6: zeros and refined = 0. */
typedef struct mantis_refine_params {
  int32_t struct_size;     /* sizeof(mantis_refine_params) */
  int32_t iterations;      /* I, 0..10 */
  int32_t half_window;     /* R, 1..15 */
  int32_t white_thresh;    /* 1..195075 */
  int32_t min_weight;      /* >= 1 */
  int32_t min_obs;         /* >= 6 */
  double lambda;           /* >= 0 */
  double landmark_pitch;   /* > 0 */
  double max_rms;          /* gate on the final rms; <= 0 means none */
  int32_t record;          /* 1 = keep every pass's rows (mantis_get_refine_record) */
  int32_t pad;
} mantis_refine_params;
/* 4 / 12 / 12288 (3 x 64^2) / 24576 / 12 / 0 / 0.08 / 0 / 0 */
void mantis_default_refine_params(mantis_refine_params* p);

typedef struct mantis_refine_result {
  int32_t status, refined, iterations_run, n_cand; /* status: 0 OK, 1 STARVED, 2 SINGULAR */
  double T_w_b[16];        /* refined base pose, row-major */
  int32_t n_obs[11];       /* per pass */
  int32_t pad;
  double rms[11];
  double delta[10][6];
  double covariance[36];
} mantis_refine_result;
/* sizeof(mantis_refine_params), sizeof(mantis_refine_result) (host only) */
void mantis_refine_sizes(int32_t* params_bytes, int32_t* result_bytes);

/* The cached line flags of the current map at `pitch` (rule above): n must be
 * nw + nr + ng, flags_out gets one byte per landmark. Host only.
 * MANTIS_ERR_ARG: no map, pitch not finite and > 0, n mismatch, null. */
mantis_status mantis_refine_line_flags(void* ctx, double pitch, uint8_t* flags_out, int32_t n);

/* n_rigs rigs of cams_per_rig cameras (cams[r * cams_per_rig + c], one frame
 * size; host or device frames, any step_bytes >= 3 W), rig r refined from
 * T_w_b_in[r] (n_rigs x 16, row-major) by the rule above. Argument limits as
 * mantis_track_batch. MANTIS_ERR_ARG (nothing launched; mantis_last_error
 * names the field): no map, n_rigs x cams_per_rig > max_cams, cams_per_rig >
 * 8, frames of different sizes, a parameter outside its range. Device work:
 * 2 (I + 1) launches on the context stream (k_refine_obs, k_refine_step per
 * pass), then one copy of the results. */
mantis_status mantis_refine_batch(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                  const double* T_w_b_in, const mantis_refine_params* p, mantis_refine_result* out);
/* One rig from the context's prior: start = prior * Transform(delta_quat,
 * delta_pos), the prior itself when motion is NULL or unset, exactly as
 * mantis_track forms its prediction. MANTIS_ERR_STATE without a prior.
 * Refined: the prior becomes T_w_b and out is a published rig (publish = 1,
 * getRotation quaternion, the covariance above, weight = final rms,
 * num_particles = final n_obs). Not refined: publish = 0, the prior stays.
 * rout (nullable) gets the details. */
mantis_status mantis_refine(void* ctx, const mantis_image* cams, int32_t n_cams, const mantis_motion* motion,
                            const mantis_refine_params* p, mantis_result* out, mantis_refine_result* rout);
/* Record of rig `rig`, pass 0 .. iterations_run of that rig, of the last
 * refine call made with record = 1; each pointer nullable: T_w_b (16) the
 * pose the pass observed at; per slot (C x n_cand, slot = c n_cand +
 * candidate) codes, Sw, Skw and rows (7 doubles each); acc28 of the pass.
 * MANTIS_ERR_STATE: no such record. MANTIS_ERR_ARG: rig or pass out of range. */
mantis_status mantis_get_refine_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, int32_t* codes,
                                       int32_t* Sw, int32_t* Skw, double* rows, double* acc28);

/* ---- Line refinement, robust rows: Huber / Tukey weights from a median ----
 * The refinement above gives every code-0 row the same weight. With this
 * switch on, each pass reweights its rows by how far their offset lies from
 * the pass's median offset (iteratively reweighted least squares), so that
 * rows which found the wrong thing -- a camera whose extrinsic has drifted, a
 * line of another colour inside the window -- pull less (Huber) or not at all
 * (Tukey). Off by default and switched per context; all addition:
 * mantis_refine_params and mantis_refine_result keep their sizes,
 * MANTIS_ABI_VERSION stays 5 (find the entries by name, check the sizes with
 * mantis_refine_robust_sizes), and with the switch off every refine entry
 * point returns the bytes it returned before.
 *
 * At every pass k = 0 .. I (the final pass included), after the observations
 * and before the accumulation, over the rig's C n_cand slots:
 *  1. key of a code-0 slot = floor(|Skw| 2^20 / Sw) in 64-bit integers: the
 *     row's offset in sample steps (about pixels, whatever fx) in units of
 *     2^-20. Sw <= 31 x 195075 < 2^23 and |Skw| <= 15 Sw, so key < 2^24
 *     (uint32). Rejected slots have key 0 and weight 0 in the record.
 *  2. n = the code-0 count, m = the key of rank floor((n - 1) / 2) in
 *     ascending order (the lower median); n = 0: m = 0. An integer: the same
 *     bits by any selection method.
 *  3. scale sigma = max(1.4826 ((double)m / 2^20), scale_floor), in steps.
 *  4. u = (double)key / 2^20, t = u / (tuning sigma).
 *     Huber: w = 1 if t <= 1, else 1 / t.
 *     Tukey: w = (1 - t t)^2 if t < 1, else 0.
 *  5. the accumulated row is sqrt(w) [J | r]: acc28 = J^T W J, J^T W r, r^T W r.
 *  6. the end of the pass as above on the weighted acc28 (rms = sqrt(r^T W r /
 *     n_obs), n_obs still the code-0 count), and STARVED also when fewer than
 *     min_obs rows have w > 0.
 *  7. the gate and the covariance as above: (r^T W r / (n_obs - 6)) (J^T W J)^-1.
 *  8. mantis_get_refine_record keeps returning the unweighted rows (its acc28
 *     is the weighted one the pass solved); keys and weights are read with
 *     mantis_get_refine_robust_record.
 * mantis_refine, mantis_refine_batch and mantis_mcl_refine_modes all take the
 * context's setting, and mantis_mcl_refine_modes' mode[k].refine stays, byte
 * for byte, mantis_refine_batch's result for the same frames and poses with
 * the switch on as with it off. Device work: k_refine_step_robust in place of
 * k_refine_step, still 2 (I + 1) launches, and one more copy back (the stats). */
typedef struct mantis_refine_robust_params {
  int32_t struct_size;  /* sizeof(mantis_refine_robust_params) */
  int32_t loss;         /* 0 none, 1 Huber, 2 Tukey */
  double tuning;        /* finite, > 0 */
  double scale_floor;   /* finite, > 0, in sample steps */
} mantis_refine_robust_params;
/* loss as given; tuning 1.345 (4.685 for loss = 2); scale_floor 0.25 */
void mantis_default_refine_robust_params(int32_t loss, mantis_refine_robust_params* p);

typedef struct mantis_refine_robust_stats {
  int32_t loss, pad;
  uint32_t median_key[11]; /* per pass; entries past iterations_run are 0 */
  int32_t n_down[11];      /* rows with w < 1 */
  int32_t n_zero[11];      /* rows with w == 0 */
  double scale[11];        /* sigma */
  double sum_w[11];        /* sum of w over the code-0 rows */
} mantis_refine_robust_stats;
/* sizeof(mantis_refine_robust_params), sizeof(mantis_refine_robust_stats) (host only) */
void mantis_refine_robust_sizes(int32_t* params_bytes, int32_t* stats_bytes);

/* The context's setting: NULL or loss = 0 switches the robust rows off (the
 * other fields are then not read). May be called any time after
 * mantis_create, is kept across calls and applies from the next refine call.
 * Host only. MANTIS_ERR_ARG (the setting stays; mantis_last_error names the
 * field): struct_size, loss outside 0..2, tuning or scale_floor not finite
 * and > 0. */
mantis_status mantis_refine_set_robust(void* ctx, const mantis_refine_robust_params* p);
/* The stats of rig `rig` of the last refine call. MANTIS_ERR_STATE: no refine
 * call yet, or the last one ran with the switch off. MANTIS_ERR_ARG: null,
 * rig out of range. */
mantis_status mantis_get_refine_robust(void* ctx, int32_t rig, mantis_refine_robust_stats* stats);
/* Keys and weights (each nullable) of rig `rig`, pass 0 .. iterations_run, of
 * the last refine call, which must have run with the switch on and record =
 * 1 (else MANTIS_ERR_STATE): one entry per slot (C x n_cand), 0 in rejected
 * slots. MANTIS_ERR_ARG: rig or pass out of range. */
mantis_status mantis_get_refine_robust_record(void* ctx, int32_t rig, int32_t pass, uint32_t* keys, double* weights);

/* ---- Monte Carlo localization: the modes refined on the grid lines ----
 * A mode of mantis_mcl_modes is a weighted mean over a cell: its resolution is
 * the particle spacing and its covariance the set's scatter. This call refines
 * every mode of the last step on that step's frames by the line refinement
 * above, unchanged, and on request moves each mode's particles rigidly so that
 * the mode's mean sits on its refined pose. All addition: no other entry
 * point, struct, kernel result or draw changes, MANTIS_ABI_VERSION stays 5
 * (find the entries by name, check the sizes with mantis_mcl_refine_sizes).
 *
 * One call, in this order:
 *  1. State and arguments. MANTIS_ERR_STATE where mantis_mcl_modes gives it (no
 *     step since the last init or reset). MANTIS_ERR_ARG: a null pointer,
 *     max_modes outside 1..8, apply not 0 or 1, and every parameter or frame
 *     error of mantis_refine_batch taken with n_rigs = 1, cams_per_rig = n_cams
 *     (mantis_last_error names the field): so n_cams <= min(8, max_cams), and
 *     the number of modes never counts against max_cams. MANTIS_ERR_STATE also
 *     for apply = 1 when an earlier apply = 1 call has moved particles since
 *     the last step (a correction is applied once; apply = 0 stays legal). On
 *     any error nothing is launched and nothing changes. cams are the frames
 *     of the step whose modes are refined, with their T_base_cam (the caller
 *     passes the right ones); host or device frames, any step_bytes >= 3 W.
 *  2. Modes. out->modes is mantis_mcl_modes(ctx, max_modes, ...)'s answer from
 *     the same state, byte for byte, and is cached the same way
 *     (mantis_mcl_select_mode may follow). After a lost step, or with n_modes =
 *     0: MANTIS_OK, no refinement is launched, every mode[k] is zero.
 *  3. Refine. Mode k < n_modes is refined from modes.mode[k].T_w_b on the
 *     n_cams frames: mode[k].refine is, byte for byte, mantis_refine_batch's
 *     result for rig k given the same frames repeated once per mode and the
 *     modes' poses as T_w_b_in. The frames are staged once and shared by all
 *     modes. p->record = 1 keeps the record (mantis_get_refine_record, rig =
 *     mode index).
 *  4. Plan (A = modes.anchor_T_w_b, g = config.grid_spacing, keys and bins as
 *     in the modes section): key_kept[k] = refine.refined && bin of
 *     key(T_ref,k, A, g) == bin of (mode k's ix, iy, yaw_quadrant); applied[k] =
 *     apply && key_kept[k]; the correction X_k = T_ref,k * inverse(T_mode,k), a
 *     rigid motion in the world frame.
 *  5. Recentre (only when some mode is applied). For each particle j of the
 *     current set (the resampled one if the step resampled, as in
 *     mantis_mcl_select_mode): b = bin of key(T_j, A, g); if an applied mode
 *     has bin b, T_j <- X_k * T_j (the plain product of the 3 x 3 bases and
 *     origins, no re-orthonormalisation); otherwise T_j keeps its bits. The
 *     log-weights, q, the prior pose and the cv::RNG state are untouched.
 *     n_moved counts the particles moved. The last step's record survives: if
 *     the current set lies in the buffer of the record's predicted poses (the
 *     step did not resample) all N particles, moved or copied, go to the other
 *     buffer, which becomes the current set; otherwise they move in place.
 *     mantis_mcl_get_record, mantis_mcl_modes, mantis_mcl_modes_color and
 *     mantis_mcl_get_color_record answer after the call exactly as before it.
 * A mode's mean is equivariant under X_k (the weights q are untouched and the
 * mean's terms turn with the poses): the moved cluster's weighted mean is
 * T_ref,k up to rounding, the rotation block of its covariance (base-frame
 * rotation vectors) is unchanged and its translation block is turned by X_k.R
 * (X_k.R Cov_t X_k.R^T). A particle near a cell boundary may change its key by
 * the move: a later mantis_mcl_select_mode keys the moved set.
 * mantis_mcl_select_mode itself is unchanged and still commits the prior to the
 * unrefined mode pose; a caller who wants the refined pose as the prior calls
 * mantis_set_prior_pose.
 * Device work, all on the context stream: the modes launch and its copy back,
 * 2 (I + 1) refinement launches and one copy back of the modes' states, then,
 * only when a mode is applied, one k_mcl_recentre launch and the copy back of
 * its 8 counters (the plan needs the refined poses and the host's gate, so it
 * is formed between the two and travels as kernel arguments). */
typedef struct mantis_mcl_mode_refined {
  int32_t applied;   /* 1: this mode's particles of the current set were moved */
  int32_t key_kept;  /* 1: the refined pose has the mode's key against the anchor */
  int32_t n_moved;   /* particles of the current set moved with this mode (0 unless applied) */
  int32_t pad;
  mantis_refine_result refine; /* of the mode's T_w_b; zeros past n_modes */
} mantis_mcl_mode_refined;
/* A tag like struct mantis_mcl_modes, which it holds: write `struct mantis_mcl_refined` in C. */
struct mantis_mcl_refined {
  int32_t status, n_modes, apply, n_moved; /* n_moved: over all modes */
  struct mantis_mcl_modes modes;           /* exactly mantis_mcl_modes's answer */
  mantis_mcl_mode_refined mode[8];         /* in mode order */
};
/* sizeof(mantis_mcl_mode_refined), sizeof(struct mantis_mcl_refined) (host only) */
void mantis_mcl_refine_sizes(int32_t* mode_bytes, int32_t* refined_bytes);
mantis_status mantis_mcl_refine_modes(void* ctx, const mantis_image* cams, int32_t n_cams, int32_t max_modes,
                                      const mantis_refine_params* p, int32_t apply, struct mantis_mcl_refined* out);

/* ---- Extrinsic calibration: joint poses + camera extrinsics on the lines ----
 * Every refine entry above takes mantis_image.T_base_cam as exact. This call
 * estimates it: from N views of one rig (N x C frames, the rig standing at N
 * places) it runs a joint Gauss-Newton over the N base poses and the
 * extrinsics of the cameras named in `free_cams`, on the grid lines, and
 * returns all of them with a covariance per free camera. All addition: no
 * other entry point, struct, kernel result or draw changes, MANTIS_ABI_VERSION
 * stays 5 (find the entries by name, check the sizes with mantis_calib_sizes).
 * The caller's mantis_images are never written; the context's prior, cv::RNG
 * state and robust setting (mantis_refine_set_robust) are neither read nor
 * changed. The refinement's robust rows do not apply here: a drifted camera
 * is modelled, not down-weighted. The calibrations have a switch of their own
 * (mantis_calib_set_robust, below) against a bad minority of rows -- one view
 * with a knocked camera, a foreign line, an occluder.
 *
 * Unknowns and the gauge. T_r = T_w_b of view r < N, and E_c = T_base_cam of
 * camera c for every bit c set in free_cams. At least one camera must be held
 * (not free) and at least one free: that fixes the gauge, and implies C >= 2.
 * The nominal extrinsic of camera c is read from view 0's cams[c].T_base_cam.
 *
 * One observation of (view r, camera c, candidate i) is exactly steps 1-8 of
 * the line refinement above (same candidates, window, codes, Sw, Skw,
 * residual), with R_cb / t_cb = inverse(E_c as currently estimated). The
 * slot's row has 13 entries [J_pose (6) | J_ext (6) | r]: J_pose is the
 * refinement's [-h | h [q]x]; J_ext belongs to the right perturbation E_c <-
 * E_c D(eps), D the update matrix of the refinement's step (Rodrigues rotation
 * eps[3..5], translation eps[0..2] taken as is): J_ext = [-g | g [p]x] with
 * g = nh^T Jpi and p the point in the camera frame (step 1). J_ext is six
 * zeros for a held camera; a rejected slot is thirteen zeros. Slot index =
 * c n_cand + candidate inside a view, no compaction.
 *
 * A pass's accumulators. Per (view, camera): acc91 = the upper triangle, row
 * by row, of M^T M for M = [J_pose | J_ext | r] (blocks PP, PE, Pr, EE, Er,
 * rr), and the count of code-0 rows. n_obs_cam[c] (over the views) and n_obs
 * are integer sums; rms = sqrt(sum rr / n_obs), the sum in (view, camera)
 * order (0 when n_obs = 0).
 *
 * The end of pass k < I:
 *  1. STARVED (1) if some view has fewer than min_obs rows over its cameras
 *     (mantis_refine_params.min_obs is per view here), or some free camera
 *     fewer than min_obs_cam rows over the views.
 *  2. per view: A_r = sum_c PP_rc + lambda I, a_r = sum_c Pr_rc (camera order).
 *  3. Cholesky of A_r (the refinement's loop); not positive definite:
 *     SINGULAR (2). Y_r = A_r^-1 [E_r | a_r], E_r = the PE blocks of the free
 *     cameras side by side in ascending camera order.
 *  4. per free camera f: B_f = sum_r EE_rf + lambda I, b_f = sum_r Er_rf.
 *  5. S = B - sum_r E_r^T A_r^-1 E_r, s = -b + sum_r E_r^T A_r^-1 a_r, every
 *     sum in view order; S is at most 42 x 42.
 *  6. left-looking Cholesky of S's lower triangle; not positive definite:
 *     SINGULAR. eps = S^-1 s.
 *  7. delta_r = -(Y_r's last column + Y_r's other columns x eps)
 *     = -A_r^-1 (a_r + E_r eps).
 *  8. T_r <- T_r D(delta_r), E_c <- E_c D(eps_c).
 * I iterations are I + 1 observation passes; the last solves nothing. I = 0
 * returns every input pose and extrinsic bit for bit. A stop ends the whole
 * call; the results keep the figures of the pass that stopped it
 * (iterations_run = the steps taken; entries past it are 0).
 *
 * Gate and covariance (host). dof = n_obs - 6 N - 6 F (F free cameras).
 * calibrated = status OK && no starved gate on the final pass && (max_rms <= 0
 * || final rms <= max_rms) && dof > 0 && S of the final pass with lambda = 0
 * positive definite. covariance[c] = (r^T r / dof) (S^-1)_cc for a free camera
 * c -- the marginal over the poses -- in the order of eps (x, y, z, rot-x,
 * rot-y, rot-z of the right perturbation), row-major; zeros for a held camera
 * and when calibrated = 0. rms_cam[c] = sqrt(sum_r rr_rc / n_obs_cam[c]) of
 * the final pass: the figure that names a drifted camera. */
typedef struct mantis_calib_params {
  int32_t struct_size;   /* sizeof(mantis_calib_params) */
  int32_t free_cams;     /* bit c: camera c's extrinsic is unknown */
  int32_t min_obs_cam;   /* >= 6 */
  int32_t pad;
} mantis_calib_params;
/* free_cams 0 (the caller names them) / min_obs_cam 60 */
void mantis_default_calib_params(mantis_calib_params* p);

typedef struct mantis_calib_result {
  int32_t status, calibrated, iterations_run, n_cand; /* status: 0 OK, 1 STARVED, 2 SINGULAR */
  int32_t n_rigs, n_cams, free_cams, pad;
  double T_base_cam[8][16];   /* the extrinsics, row-major; the input bytes for held cameras; zeros past n_cams */
  int32_t n_obs[11];          /* per pass */
  int32_t pad2;
  int32_t n_obs_cam[11][8];
  double rms[11];
  double rms_cam[8];          /* of the final pass */
  double delta_cam[10][8][6]; /* eps per pass and camera; zeros for held cameras */
  double covariance[8][36];
} mantis_calib_result;
/* sizeof(mantis_calib_params), sizeof(mantis_calib_result) (host only) */
void mantis_calib_sizes(int32_t* params_bytes, int32_t* result_bytes);

/* n_rigs views of one rig of cams_per_rig cameras (cams[r * cams_per_rig + c]
 * as in mantis_refine_batch), view r starting from T_w_b_in[r] (n_rigs x 16).
 * The window, gates, lambda, pitch, iterations and `record` come from p.
 * T_w_b_out (n_rigs x 16) gets the views' poses, out the rest. Limits and
 * errors as mantis_refine_batch, and MANTIS_ERR_ARG (nothing launched;
 * mantis_last_error names the field) for: n_rigs > 256, cams_per_rig < 2,
 * free_cams empty, free_cams naming every camera, free_cams with a bit at or
 * above cams_per_rig, min_obs_cam < 6, a T_base_cam that is not finite, a
 * view whose cams[c].T_base_cam differs from view 0's in any byte. Device
 * work: 3 (I + 1) launches on the context stream (k_calib_obs, k_calib_rig,
 * k_calib_solve per pass), then the copies of the results. */
mantis_status mantis_calibrate_extrinsics(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                          const double* T_w_b_in, const mantis_refine_params* p,
                                          const mantis_calib_params* cp, double* T_w_b_out, mantis_calib_result* out);
/* Record of view `rig`, pass 0 .. iterations_run, of the last calibration made
 * with p->record = 1; each pointer nullable: T_w_b (16) and T_base_cam (C x
 * 16) the pass observed at; per slot (C x n_cand) codes, Sw, Skw and rows (13
 * doubles each); acc91 (C x 91) of the view. MANTIS_ERR_STATE: no such record.
 * MANTIS_ERR_ARG: rig or pass out of range. */
mantis_status mantis_get_calib_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, double* T_base_cam,
                                      int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, double* acc91);

/* ---- Intrinsic calibration: joint poses + K and fisheye D on the lines ----
 * Every entry above that works on the grid lines takes mantis_image.K and
 * mantis_image.D as exact. This call estimates them: from N views of one rig
 * it runs a joint Gauss-Newton over the N base poses and the eight intrinsics
 * (fx, fy, cx, cy, k1..k4) of the cameras named in `free_cams`, on the grid
 * lines, and returns all of them with a covariance per free camera. All
 * addition: no other entry point, struct, kernel result or draw changes,
 * MANTIS_ABI_VERSION stays 5 (find the entries by name, check the sizes with
 * mantis_icalib_sizes). The caller's mantis_images are never written; the
 * context's prior, cv::RNG state and robust setting are neither read nor
 * changed. The extrinsics are held at cams[c].T_base_cam: a caller who needs
 * both calls mantis_calibrate_rig (below), which solves for them together
 * (alternating this call with mantis_calibrate_extrinsics does not converge).
 *
 * Unknowns. T_r = T_w_b of view r < N, and theta_c = (fx, fy, cx, cy, k1, k2,
 * k3, k4) of every camera c named in free_cams. There is no gauge freedom (the
 * map fixes the world, the extrinsics are held): free_cams may name every
 * camera and C = 1 is legal. The start of theta_c is view 0's cams[c].K
 * (rounded to float, as every other entry does) and cams[c].D (as given);
 * every view's K and D of camera c must equal view 0's byte for byte. From
 * then on theta lives in FP64 in the call's device state. A result fed back
 * through mantis_image.K is rounded to float there: 6e-8 relative, harmless.
 *
 * Which parameters are free. param_mask bit i frees parameter i (in the order
 * above, 0xFF = all) of every free camera. A held parameter's J_int column is
 * zero in every row, its diagonal entry of B_f is set to exactly 1 after
 * lambda is added, and its update is skipped: the value comes back bit for bit.
 *
 * One observation of (view r, camera c, candidate i) is exactly steps 1-8 of
 * the line refinement (same candidates, window, codes, Sw, Skw, J_pose), with
 * Cam = the current theta_c and the sample step s = 1 / fx of the current FP64
 * estimate; r = -((double)Skw / (double)Sw) s. The slot's row has 15 entries
 * [J_pose (6) | J_int (8) | r]; a rejected slot is fifteen zeros, a held
 * camera has eight zeros for J_int. Slot index = c n_cand + candidate inside a
 * view, no compaction.
 *
 * J_int belongs to the relative perturbation eps (8): fx <- fx (1 + eps0),
 * fy <- fy (1 + eps1), cx <- cx + fx eps2, cy <- cy + fy eps3 (fx, fy before
 * the update), k_i <- k_i + eps_(3+i). At m = m0 = (x, y) (step 1), rho = |m|,
 * t = atan rho, t_d = t + k1 t^3 + k2 t^5 + k3 t^7 + k4 t^9,
 * t_d' = 1 + 3 k1 t^2 + 5 k2 t^4 + 7 k3 t^6 + 9 k4 t^8, c = t_d / rho,
 * c' = (t_d' / (1 + rho^2) - c) / rho, G = c I + (c' / rho) m m^T (the
 * derivative of the normalized distortion), Q (2 x 8) with the columns
 * (c x, 0), (0, c y), (1, 0), (0, 1), m t^3 / rho, m t^5 / rho, m t^7 / rho,
 * m t^9 / rho: J_int = nh^T G^-1 Q, G inverted in closed form. For rho <= 1e-8
 * (distort's own branch) G = I, c = 1 and the k columns are zero. (The line
 * was seen at a fixed pixel P = dist(m_obs) and r = nh . (m0 - m_obs), so
 * dr/dtheta = nh^T (d dist / d m)^-1 d dist / d theta.)
 *
 * A pass's accumulators. Per (view, camera): acc120 = the upper triangle, row
 * by row, of M^T M for M = [J_pose | J_int | r] (blocks PP, PI, Pr, II, Ir,
 * rr), and the count of code-0 rows. n_obs, n_obs_cam and rms as in the
 * extrinsic calibration (integer sums; rr summed in (view, camera) order).
 *
 * The end of pass k < I is the extrinsic calibration's steps 1-8 with 8 in
 * place of 6 for the camera blocks: the two starved gates (min_obs per view,
 * min_obs_cam per free camera over the views; STARVED = 1), A_r = sum_c PP_rc
 * + lambda I and its 6 x 6 Cholesky (SINGULAR = 2), Y_r = A_r^-1 [E_r | a_r]
 * with E_r the PI blocks of the free cameras in ascending order (6 x 8 F),
 * B_f = sum_r II_rf + lambda I (held parameters: see above), b_f = sum_r
 * Ir_rf, S = B - sum_r E_r^T Y_r^E, s = -b + sum_r E_r^T Y_r^a (view order; S
 * is at most 64 x 64), the left-looking Cholesky of S's lower triangle
 * (SINGULAR), eps = S^-1 s, delta_r = -(Y_r^a + Y_r^E eps), T_r <- T_r
 * D(delta_r), theta_c updated as above. If an updated fx or fy is not finite
 * or <= 0, or any updated parameter is not finite: DIVERGED (3); the call
 * stops and keeps the poses and parameters from before that step. I
 * iterations are I + 1 observation passes; the last solves nothing. I = 0
 * returns every pose bit for bit, every K as the float-rounded input and D as
 * given. A stop ends the whole call (iterations_run = the steps taken;
 * entries past it are 0).
 *
 * Gate and covariance (host). dof = n_obs - 6 N - P, P the number of free
 * parameters over the free cameras. calibrated = status OK && no starved gate
 * on the final pass && (max_rms <= 0 || final rms <= max_rms) && dof > 0 && S
 * of the final pass with lambda = 0 positive definite. covariance[c] (8 x 8,
 * row-major) = (r^T r / dof) (S^-1)_cc scaled by diag(fx, fy, fx, fy, 1, 1, 1,
 * 1) on both sides: px^2 for K, dimensionless for D. Zeros in a held
 * parameter's row and column, for a held camera and when calibrated = 0.
 * rms_cam[c] of the final pass as in the extrinsic calibration. */
typedef struct mantis_icalib_params {
  int32_t struct_size;   /* sizeof(mantis_icalib_params) */
  int32_t free_cams;     /* bit c: camera c's intrinsics are unknown */
  int32_t param_mask;    /* bit i: parameter i (fx, fy, cx, cy, k1..k4) is free; 1..0xFF */
  int32_t min_obs_cam;   /* >= 8 */
} mantis_icalib_params;
/* free_cams 0 (the caller names them) / param_mask 0xFF / min_obs_cam 60 */
void mantis_default_icalib_params(mantis_icalib_params* p);

typedef struct mantis_icalib_result {
  int32_t status, calibrated, iterations_run, n_cand; /* status: 0 OK, 1 STARVED, 2 SINGULAR, 3 DIVERGED */
  int32_t n_rigs, n_cams, free_cams, param_mask;
  double K[8][4];             /* fx, fy, cx, cy; the (float-rounded) input for held cameras; zeros past n_cams */
  double D[8][4];             /* k1..k4 */
  int32_t n_obs[11];          /* per pass */
  int32_t pad;
  int32_t n_obs_cam[11][8];
  double rms[11];
  double rms_cam[8];          /* of the final pass */
  double delta_cam[10][8][8]; /* eps per pass and camera; zeros for held cameras and held parameters */
  double covariance[8][64];
} mantis_icalib_result;
/* sizeof(mantis_icalib_params), sizeof(mantis_icalib_result) (host only) */
void mantis_icalib_sizes(int32_t* params_bytes, int32_t* result_bytes);

/* n_rigs views of one rig of cams_per_rig cameras, laid out and started as in
 * mantis_calibrate_extrinsics; the window, gates, lambda, pitch, iterations
 * and `record` come from p. Limits and errors are those of
 * mantis_calibrate_extrinsics (MANTIS_ERR_ARG, nothing launched,
 * mantis_last_error names the field), except: cams_per_rig >= 1; free_cams
 * may name every camera, but not none and no bit at or above cams_per_rig;
 * param_mask in 1..0xFF; min_obs_cam >= 8; a K or D that is not finite, or
 * fx or fy <= 0; a view whose K, D or T_base_cam differs from view 0's in any
 * byte. Device work: 3 (I + 1) launches on the context stream (k_icalib_obs,
 * k_icalib_rig, k_icalib_solve per pass), then the copies of the results. */
mantis_status mantis_calibrate_intrinsics(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                          const double* T_w_b_in, const mantis_refine_params* p,
                                          const mantis_icalib_params* ip, double* T_w_b_out, mantis_icalib_result* out);
/* Record of view `rig`, pass 0 .. iterations_run, of the last intrinsic
 * calibration made with p->record = 1; each pointer nullable: T_w_b (16) and
 * KD (C x 8: fx, fy, cx, cy, k1..k4) the pass observed at; per slot (C x
 * n_cand) codes, Sw, Skw and rows (15 doubles each); acc120 (C x 120) of the
 * view. MANTIS_ERR_STATE: no such record. MANTIS_ERR_ARG: rig or pass out of
 * range. */
mantis_status mantis_get_icalib_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, double* KD, int32_t* codes,
                                       int32_t* Sw, int32_t* Skw, double* rows, double* acc120);

/* ---- Rig calibration: poses + extrinsics + intrinsics in one solve ----
 * mantis_calibrate_extrinsics takes every K and D as exact,
 * mantis_calibrate_intrinsics every T_base_cam. On a rig where neither is
 * exact each of them absorbs the other's error into its own unknowns, and
 * alternating them does not converge to the rig (DESIGN 4j has the figures).
 * This call estimates all of it at once: from N views of one rig it runs a
 * joint Gauss-Newton over the N base poses, the extrinsics of the cameras
 * named in `free_ext` and the eight intrinsics of the cameras named in
 * `free_int`, on the grid lines. All addition: no other entry point, struct,
 * kernel result or draw changes, MANTIS_ABI_VERSION stays 5 (find the entries
 * by name, check the sizes with mantis_rcalib_sizes). The caller's
 * mantis_images are never written; the context's prior, cv::RNG state and
 * robust setting are neither read nor changed.
 *
 * Unknowns. T_r = T_w_b of view r < N (N <= 256); E_c = T_base_cam of every
 * camera in free_ext; theta_c = (fx, fy, cx, cy, k1..k4) of every camera in
 * free_int. Both masks must name a camera. Gauge as in the extrinsic
 * calibration: free_ext must leave at least one camera held (so C >= 2);
 * free_int may name every camera. param_mask has the intrinsic calibration's
 * meaning, the exact 1 on a held parameter's diagonal included. Starts: view
 * 0's T_base_cam, K rounded to float, D as given; every view's T_base_cam, K
 * and D must equal view 0's byte for byte.
 *
 * One observation is the intrinsic calibration's, taken at the current theta_c
 * and at R_cb / t_cb = inverse(current E_c), with the sample step s = 1 / fx
 * of the current estimate. The slot's row has 21 entries
 * [J_pose (6) | J_ext (6) | J_int (8) | r]: J_ext is the extrinsic
 * calibration's [-g | g [p]x] from the same geometry, J_int the intrinsic
 * calibration's. A camera held in a mask has zeros in that block; a rejected
 * slot is 21 zeros. With free_int's bit clear (and a float-representable K)
 * columns 0-11 and 20, the codes and the sums equal the extrinsic
 * calibration's slot bit for bit; with free_ext's bit clear columns 0-5 and
 * 12-20 equal the intrinsic calibration's.
 *
 * A pass's accumulators. Per (view, camera): acc231 = the upper triangle, row
 * by row, of M^T M for M = [J_pose | J_ext | J_int | r] (blocks PP, PE, PI,
 * Pr, EE, EI, Er, II, Ir, rr), and the count of code-0 rows. n_obs, n_obs_cam
 * and rms as in the other two calibrations.
 *
 * The end of pass k < I is the extrinsic calibration's steps 1-8. The reduced
 * unknowns are the extrinsic blocks of free_ext (ascending cameras, 6 each),
 * then the intrinsic blocks of free_int (ascending, 8 each): nS = 6 Fe + 8 Fi
 * <= 106. Both starved gates apply, min_obs_cam to a camera free in either
 * mask (STARVED = 1). A_r = sum_c PP_rc + lambda I and its 6 x 6 Cholesky
 * (SINGULAR = 2); [E_r | a_r] (6 x (nS + 1)) = the PE and PI blocks of the
 * free cameras in the order above and sum_c Pr_rc; Y_r = A_r^-1 [E_r | a_r].
 * B is block diagonal per camera: EE (+ lambda I) and II (+ lambda I; a held
 * parameter's diagonal entry exactly 1) summed over the views, and for a
 * camera free in both masks the off-diagonal block sum_r EI. b = the Er and
 * Ir sums. S = B - sum_r E_r^T Y_r^E, s = -b + sum_r E_r^T Y_r^a, every sum in
 * view order; the left-looking Cholesky of S's lower triangle (SINGULAR);
 * eps = S^-1 s; delta_r = -(Y_r^a + Y_r^E eps); T_r <- T_r D(delta_r), E_c <-
 * E_c D(eps_c), theta_c updated as in the intrinsic calibration. If an updated
 * fx or fy is not finite or <= 0, or any updated parameter is not finite:
 * DIVERGED (3); the call stops and keeps the poses, extrinsics and parameters
 * from before that step. I = 0 returns every pose and extrinsic bit for bit,
 * K as the float-rounded input and D as given.
 *
 * Gate and covariance (host). dof = n_obs - 6 N - 6 Fe - P, P the number of
 * free parameters over the cameras of free_int. calibrated = status OK && no
 * starved gate on the final pass && (max_rms <= 0 || final rms <= max_rms) &&
 * dof > 0 && S of the final pass with lambda = 0 positive definite.
 * cov_ext[c] (6 x 6) and cov_int[c] (8 x 8, scaled by diag(fx, fy, fx, fy, 1,
 * 1, 1, 1) on both sides) are the diagonal blocks of (r^T r / dof) S^-1.
 * Zeros where held and when calibrated = 0. */
typedef struct mantis_rcalib_params {
  int32_t struct_size;   /* sizeof(mantis_rcalib_params) */
  int32_t free_ext;      /* bit c: camera c's extrinsic is unknown; at least one camera held */
  int32_t free_int;      /* bit c: camera c's intrinsics are unknown */
  int32_t param_mask;    /* bit i: parameter i (fx, fy, cx, cy, k1..k4) is free; 1..0xFF */
  int32_t min_obs_cam;   /* >= 14 */
  int32_t pad;
} mantis_rcalib_params;
/* free_ext 0 / free_int 0 (the caller names them) / param_mask 0xFF / min_obs_cam 60 */
void mantis_default_rcalib_params(mantis_rcalib_params* p);

typedef struct mantis_rcalib_result {
  int32_t status, calibrated, iterations_run, n_cand; /* status: 0 OK, 1 STARVED, 2 SINGULAR, 3 DIVERGED */
  int32_t n_rigs, n_cams, free_ext, free_int;
  int32_t param_mask, pad;
  double T_base_cam[8][16];   /* row-major; the input for cameras held in free_ext; zeros past n_cams */
  double K[8][4];             /* fx, fy, cx, cy; the (float-rounded) input for cameras held in free_int */
  double D[8][4];             /* k1..k4 */
  int32_t n_obs[11];          /* per pass */
  int32_t pad2;
  int32_t n_obs_cam[11][8];
  double rms[11];
  double rms_cam[8];          /* of the final pass */
  double delta_ext[10][8][6]; /* eps per pass and camera; zeros where held */
  double delta_int[10][8][8];
  double cov_ext[8][36];
  double cov_int[8][64];
} mantis_rcalib_result;
/* sizeof(mantis_rcalib_params), sizeof(mantis_rcalib_result) (host only) */
void mantis_rcalib_sizes(int32_t* params_bytes, int32_t* result_bytes);

/* n_rigs views of one rig of cams_per_rig cameras, laid out and started as in
 * the other two calibrations; the window, gates, lambda, pitch, iterations and
 * `record` come from p. Errors (MANTIS_ERR_ARG, nothing launched,
 * mantis_last_error names the field): those of mantis_calibrate_extrinsics
 * and mantis_calibrate_intrinsics together, with free_ext and free_int in
 * place of free_cams: either mask empty or with a bit at or above
 * cams_per_rig, free_ext naming every camera, min_obs_cam < 14.
 * MANTIS_ERR_STATE: the device refused the solve kernel's LDS. Device work:
 * 3 (I + 1) launches on the context stream (k_rcalib_obs, k_rcalib_rig,
 * k_rcalib_solve per pass), then the copies of the results. */
mantis_status mantis_calibrate_rig(void* ctx, const mantis_image* cams, int32_t n_rigs, int32_t cams_per_rig,
                                   const double* T_w_b_in, const mantis_refine_params* p,
                                   const mantis_rcalib_params* rp, double* T_w_b_out, mantis_rcalib_result* out);
/* Record of view `rig`, pass 0 .. iterations_run, of the last rig calibration
 * made with p->record = 1; each pointer nullable: T_w_b (16), T_base_cam (C x
 * 16) and KD (C x 8) the pass observed at; per slot (C x n_cand) codes, Sw,
 * Skw and rows (21 doubles each); acc231 (C x 231) of the view.
 * MANTIS_ERR_STATE: no such record. MANTIS_ERR_ARG: rig or pass out of range. */
mantis_status mantis_get_rcalib_record(void* ctx, int32_t rig, int32_t pass, double* T_w_b, double* T_base_cam,
                                       double* KD, int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows,
                                       double* acc231);

/* ---- Calibration, robust rows: Huber / Tukey weights from a call-wide median ----
 * The three calibrations above give every code-0 row the same weight, and what
 * they return is taken as exact by every later call: a camera knocked in one of
 * the N views, a foreign line or an occluder in one frame ends up in
 * T_base_cam, K and D. With this switch on, every pass reweights its rows as
 * the line refinement's robust rows do, but from one scale over the whole call
 * (all views and cameras): one joint solve has one noise scale, and a median
 * per view would be blind to a view that is wrong as a whole. Off by default
 * and switched per context; all addition: no struct above changes its size,
 * MANTIS_ABI_VERSION stays 5 (find the entries by name, check the sizes with
 * mantis_calib_robust_sizes), and with the switch off the three calibrations
 * return the bytes they returned before and launch the kernels they launched
 * before. The switch is independent of mantis_refine_set_robust in both
 * directions.
 *
 * At every pass k = 0 .. I, after the observations and before the accumulation:
 *  1. key of a code-0 slot = floor(|Skw| 2^20 / Sw), the refinement's key.
 *     Rejected slots have key 0 and weight 0 in the record.
 *  2. n = the code-0 count over all N C n_cand slots of the call, m = the key
 *     of rank floor((n - 1) / 2) among them in ascending order; n = 0: m = 0.
 *  3. sigma = max(1.4826 ((double)m / 2^20), scale_floor).
 *  4. w = the refinement's weight of (key, loss, tuning, sigma).
 *  5. the accumulated row is sqrt(w) [J ... | r], all 13, 15 or 21 columns.
 *  6. n_obs, n_obs_cam and the record's rows stay the unweighted code-0
 *     figures; rms, rms_cam, the covariances and every solve take the weighted
 *     accumulators (rms = sqrt(r^T W r / n_obs)).
 *  7. STARVED also when a view has fewer than min_obs rows with w > 0,
 *  8. and when a camera free in either mask has fewer than min_obs_cam rows
 *     with w > 0. Both also clear `calibrated` on the final pass.
 *  9. the end of the pass, dof, the gate and the covariances are otherwise
 *     those of the calibration, on the weighted accumulators.
 * 10. I = 0 returns every input bit for bit; the stats of pass 0 are filled.
 * Device work with the switch on: 5 (I + 1) launches (k_*_obs, k_*_hist twice,
 * k_*_rig, k_*_solve per pass; the selection of m spans the views' blocks and
 * every hand-off is a kernel boundary), one memset of the selection tables
 * before the first pass and one more copy back (the stats). */
typedef struct mantis_calib_robust_stats {
  int32_t loss, kind;          /* kind: 0 extrinsic, 1 intrinsic, 2 rig */
  int32_t n_rigs, n_cams;
  uint32_t median_key[11];     /* per pass; entries past iterations_run are 0 */
  int32_t n_down[11];          /* rows with w < 1, over the call */
  int32_t n_zero[11];          /* rows with w == 0 */
  int32_t pad;
  double scale[11];            /* sigma */
  double sum_w[11];            /* sum of w over the code-0 rows, in (view, camera) order */
  /* of the last pass run (iterations_run); zeros past n_rigs / n_cams */
  int32_t n_obs_view[256];     /* code-0 rows of the view over its cameras */
  int32_t n_zero_view[256];
  double sum_w_view[256];      /* a wrong view has a low sum_w_view / n_obs_view */
  int32_t n_zero_cam[8];
  double sum_w_cam[8];         /* against n_obs_cam[iterations_run][c] of the result */
} mantis_calib_robust_stats;
/* sizeof(mantis_refine_robust_params) (the parameters are the refinement's
 * struct), sizeof(mantis_calib_robust_stats) (host only) */
void mantis_calib_robust_sizes(int32_t* params_bytes, int32_t* stats_bytes);

/* The context's setting for all three calibrations: NULL or loss = 0 switches
 * the robust rows off. Defaults: mantis_default_refine_robust_params. Kept
 * across calls, applies from the next calibration. Host only. MANTIS_ERR_ARG
 * (the setting stays; mantis_last_error names the field): struct_size, loss
 * outside 0..2, tuning or scale_floor not finite and > 0. */
mantis_status mantis_calib_set_robust(void* ctx, const mantis_refine_robust_params* p);
/* The stats of the last calibration of `kind` (0 extrinsic, 1 intrinsic, 2
 * rig; each kind keeps its own). MANTIS_ERR_STATE: no call of that kind yet,
 * or its last call ran with the switch off. MANTIS_ERR_ARG: null, kind outside
 * 0..2. */
mantis_status mantis_get_calib_robust(void* ctx, int32_t kind, mantis_calib_robust_stats* stats);
/* Keys and weights (each nullable) of view `rig`, pass 0 .. iterations_run, of
 * the last calibration of `kind`, which must have run with the switch on and
 * record = 1 (else MANTIS_ERR_STATE): one entry per slot (C x n_cand), 0 in
 * rejected slots. mantis_get_calib_record and its two siblings keep returning
 * the unweighted rows; their accumulators are the weighted ones the pass
 * solved. MANTIS_ERR_ARG: kind, rig or pass out of range. */
mantis_status mantis_get_calib_robust_record(void* ctx, int32_t kind, int32_t rig, int32_t pass, uint32_t* keys,
                                             double* weights);

/* ---- Window smoothing: line rows plus odometry factors over N views ----
 * Every refine and calibration entry above treats the views of a call as
 * independent rig poses. This call ties N consecutive views of one rig
 * together with the service's motions (mantis_motion) and solves the short
 * trajectory jointly: a view that sees too few lines (STARVED on its own) is
 * held by its factors, and every view gets a marginal covariance that accounts
 * for the odometry. All addition: no other entry point, struct, kernel result
 * or draw changes, MANTIS_ABI_VERSION stays 5 (find the entries by name, check
 * the sizes with mantis_smooth_sizes). Nothing is drawn from the cv::RNG, the
 * context's prior pose is not touched, and the robust switches
 * (mantis_refine_set_robust, mantis_calib_set_robust) are not read.
 *
 * A window: N views (1 <= N <= 256) of one rig of C cameras (1..8), frames
 * cams[(w N + k) C + c], one size. View k starts at T_w_b_in[k]. Step k -> k+1
 * (k = 0 .. N - 2) has motions[k]; Delta_k = Transform(delta_quat, delta_pos),
 * formed as mantis_track / mantis_refine form their prediction, so T_k+1 ~
 * T_k Delta_k. An unset motion (|q|^2 < 0.5) puts no factor on its step: the
 * chain breaks there and the two sides are independent segments of one system.
 *
 * Rows: exactly the line refinement's (codes, Sw, Skw, the 7-column row, slot
 * = c n_cand + candidate). Per view A_k = J^T J, b_k = J^T r, r^T r (acc28)
 * and n_obs_k. The line rows keep unit weight.
 *
 * Between factor of a set motion k, with the right perturbation T <- T D(x)
 * of the refinement's step: M = T_k^-1 T_k+1 = [R_M | t_M], E = Delta_k^-1 M
 * = [R_E | t_E], e = [t_E ; log R_E] (translation as is, rotation vector),
 *   de/dx_k+1 = [[R_E, 0], [0, Jri]],
 *   de/dx_k   = [[-R_D^T, R_D^T [t_M]x], [0, -Jri R_M^T]],
 *   Jri = J_r^-1(e_r) = I + [phi]x / 2 + (1 / th^2 - (1 + cos th) / (2 th sin
 *   th)) [phi]x^2, and I + [phi]x / 2 + [phi]x^2 / 12 for th < 1e-8.
 * Whitening: rows 0..2 of e and of both Jacobians times sigma_row / sigma_t,
 * rows 3..5 times sigma_row / sigma_rot.
 * Prior factor (optional, view 0): e_p = [t_0 - t_p ; log(R_p^T R_0)],
 * de_p/dx_0 = [[R_0, 0], [0, Jri]], whitened by sigma_row L_c^-1 with
 * prior_cov = L_c L_c^T (Cholesky, host); prior_cov has the order and frames
 * of mantis_refine_result.covariance (translation in the world frame, rotation
 * a right perturbation).
 *
 * System of a pass, block tridiagonal in 6 x 6 blocks, every term added in
 * this order: H_kk = A_k + Jb^T Jb (factor k - 1) + Ja^T Ja (factor k) + the
 * prior's (k = 0) + lambda I; H_k+1,k = Jb^T Ja (factor k); g_k likewise from
 * b_k and the J^T e terms (Ja = de/dx_k, Jb = de/dx_k+1, whitened). Solve by
 * block Cholesky: L_kk = chol(H_kk - L_k,k-1 L_k,k-1^T), L_k+1,k = H_k+1,k
 * L_kk^-T, forward and back substitution, every dot product in ascending index
 * order; x = -H^-1 g, T_k <- T_k D(x_k).
 *
 * Pass p = 0 .. I: n_obs[p] = sum of the views' n_obs in view order, rms[p] =
 * sqrt(r^T r / n_obs) over the rows only, motion_rms[p] = sqrt(sum e^T e / (6
 * n_factors)) / sigma_row (about 1 when the odometry is as good as its sigmas
 * say; 0 without factors), cost[p] = r^T r + sum e^T e (+ the prior's).
 * STARVED when the window's n_obs < min_obs, SINGULAR when a diagonal block is
 * not positive definite; either stops the whole window, which keeps the
 * figures of the pass that stopped it at index iterations_run. A single blind
 * view stops nothing. Pass I observes and solves nothing: I = 0 returns every
 * input pose bit for bit.
 *
 * Gate and covariances (host, on the final pass's blocks at lambda = 0): dof =
 * n_obs + 6 n_factors + 6 has_prior - 6 N, sigma2 = cost / dof; the marginals
 * S_k are the diagonal blocks of H^-1 by the backward recursion S_N-1 = (L
 * L^T)^-1, S_k = (L_kk L_kk^T)^-1 + G_k^T S_k+1 G_k, G_k = L_k+1,k L_kk^-1;
 * covariance_k = sigma2 S_k with the translation block turned to the world
 * frame by R_wb,k. smoothed = status OK && n_obs >= min_obs && (max_rms <= 0
 * || rms <= max_rms) && dof > 0 && every block positive definite; otherwise
 * the covariances are zeros. */
typedef struct mantis_smooth_params {
  int32_t struct_size;     /* sizeof(mantis_smooth_params) */
  int32_t iterations;      /* I, 0..10 */
  int32_t half_window;     /* R, 1..15 */
  int32_t white_thresh;    /* 1..195075 */
  int32_t min_weight;      /* >= 1 */
  int32_t min_obs;         /* >= 6, of the window */
  double lambda;           /* >= 0 */
  double landmark_pitch;   /* > 0 */
  double max_rms;          /* gate on the final rms; <= 0 means none */
  double sigma_row;        /* finite and > 0: one line row, normalized image units */
  double sigma_t;          /* finite and > 0: a step's translation, map units */
  double sigma_rot;        /* finite and > 0: a step's rotation, rad */
  int32_t record;          /* 1 = keep every pass (mantis_get_smooth_record / _pass) */
  int32_t pad;
} mantis_smooth_params;
/* the refine defaults, then 0.00127 / 0.01 / 0.03 (0.41 px over fx = 323.15;
 * mantis_mcl_params' per-step sigma_t / sigma_rot) */
void mantis_default_smooth_params(mantis_smooth_params* p);

typedef struct mantis_smooth_result { /* per window */
  int32_t status, smoothed, iterations_run, n_cand; /* status: 0 OK, 1 STARVED, 2 SINGULAR */
  int32_t n_views, n_factors, has_prior, dof;
  int32_t n_obs[11];       /* per pass, of the window */
  int32_t pad;
  double rms[11];
  double motion_rms[11];
  double cost[11];
  double sigma2;
} mantis_smooth_result;
typedef struct mantis_smooth_view { /* per window x view */
  int32_t n_obs, pad;      /* of the last pass taken */
  double rms;
  double T_w_b[16];        /* smoothed base pose, row-major */
  double covariance[36];   /* x, y, z, rot-x, rot-y, rot-z, row-major */
} mantis_smooth_view;
/* sizeof(mantis_smooth_params), sizeof(mantis_smooth_result), sizeof(mantis_smooth_view) (host only) */
void mantis_smooth_sizes(int32_t* params_bytes, int32_t* result_bytes, int32_t* view_bytes);

/* n_windows windows of n_views views by the rule above. T_w_b_in: n_windows x
 * n_views x 16. motions: n_windows x (n_views - 1), NULL only when n_views ==
 * 1. prior_T (n_windows x 16, nullable) with prior_cov (n_windows x 36, not
 * null when prior_T is). out: per window; views: per window x view.
 * MANTIS_ERR_ARG (nothing launched; mantis_last_error names the field): no
 * map, n_windows x n_views x cams_per_rig > max_cams, n_views > 256,
 * cams_per_rig > 8, frames of different sizes, a parameter outside its range,
 * a pose or motion that is not finite, a prior covariance that is not finite
 * or not positive definite, a null pointer. Device work: 3 (I + 1) launches on
 * the context stream (k_refine_obs as it is with views as its rigs,
 * k_smooth_acc, k_smooth_solve per pass), then one copy of the results. */
mantis_status mantis_smooth_batch(void* ctx, const mantis_image* cams, int32_t n_windows, int32_t n_views,
                                  int32_t cams_per_rig, const double* T_w_b_in, const mantis_motion* motions,
                                  const double* prior_T, const double* prior_cov, const mantis_smooth_params* p,
                                  mantis_smooth_result* out, mantis_smooth_view* views);
/* Record of view `view` of window `window`, pass 0 .. iterations_run of that
 * window, of the last smooth call made with record = 1: the shape of
 * mantis_get_refine_record. MANTIS_ERR_STATE: no such record. MANTIS_ERR_ARG:
 * an index out of range. */
mantis_status mantis_get_smooth_record(void* ctx, int32_t window, int32_t view, int32_t pass, double* T_w_b,
                                       int32_t* codes, int32_t* Sw, int32_t* Skw, double* rows, double* acc28);
/* The pass-level record, each pointer nullable: e ((N - 1) x 6, whitened,
 * zeros where no factor), J ((N - 1) x 72: Ja | Jb, whitened), prior_e (6),
 * prior_J (36), delta (N x 6: the step the pass took; zeros on the pass that
 * ended the window). Errors as mantis_get_smooth_record. */
mantis_status mantis_get_smooth_pass(void* ctx, int32_t window, int32_t pass, double* e, double* J, double* prior_e,
                                     double* prior_J, double* delta);

/* ---- Fixed-lag smoothing: a context-held window that marginalises ----
 * mantis_smooth_batch is a batch call: the caller holds N views of frames and
 * re-stages all of them on every call. These entries keep the window in the
 * context (in HBM, as the MCL set): one call per incoming view, and the
 * information of the view that leaves is carried forward as a Gaussian prior
 * on the next one, computed on the device by a Schur complement. All addition:
 * no other entry point, struct, kernel or draw changes, MANTIS_ABI_VERSION
 * stays 5 (find the entries by name, check the sizes with mantis_lag_sizes).
 * Nothing is drawn from the cv::RNG; the context's prior pose and the robust
 * switches are not touched. Other entries may be called between pushes: the
 * window has its own frames, descriptors and workspaces.
 *
 * mantis_lag_reset empties the window and fixes its shape: capacity N (2..256),
 * cams_per_rig C (1..8, <= max_cams; the N C frames the window keeps do not
 * count against max_cams) and the smoothing parameters. prior_T (16) with
 * prior_cov (36), both nullable together, put a prior on the first view; they
 * are checked as mantis_smooth_batch checks its prior. Nothing is launched.
 *
 * mantis_lag_push appends one view of C frames (cams[c], one size, the size of
 * the first push since the reset; copied into the window's own ring of N C
 * frames, so the caller's buffers are free when the push returns). motion: the
 * step from the newest held view to this one (ignored on the first push, where
 * it may be NULL); an unset motion (|q|^2 < 0.5) puts no factor there. T_start
 * (16, nullable): where the view starts; NULL: T_newest Delta, formed on the
 * device by the product of the MCL and track predictions; required on the
 * first push and after an unset motion. When the window already held N views,
 * the oldest is first marginalised into a prior on the next one and the rest
 * shift down:
 *   from the last push's final pass (the lambda = 0 blocks of pass
 *   iterations_run, with the factors and the prior of that same pass), H_00 and
 *   g_0 as assembled and factor 0's whitened Ja, Jb, e:
 *   Lambda = Jb^T Jb - (Jb^T Ja) H_00^-1 (Ja^T Jb), eta = Jb^T e - (Jb^T Ja)
 *   H_00^-1 g_0 (Cholesky of H_00, two triangular solves, every dot product in
 *   ascending index order), x* = -Lambda^-1 eta, T_p = T_1 D(x*), Cov_p =
 *   sigma_row^2 Lambda^-1 with the translation and cross blocks turned to the
 *   world frame by R of T_p; symmetric bit for bit. (T_p, Cov_p) has the shape
 *   and frames of mantis_smooth_batch's prior_T / prior_cov, and its whitener
 *   is formed on the device as that call's host forms it.
 * This is a first-order marginal at the leaving view's final linearisation
 * point; no first-estimate Jacobians are kept. No prior is carried (drop_reason
 * says why) when step 0 had no factor (1), the last push did not end OK (2), or
 * H_00 (3), Lambda (4) or Cov_p (5) is not positive definite or not finite.
 * Then the passes of mantis_smooth_batch run over the views held, each from
 * the pose it held (the new one from its start): the same kernels on the same
 * bytes, so a push returns what mantis_smooth_batch returns for those views,
 * starts, motions and prior. out_views: `capacity` entries, the first
 * out_result->n_views valid, newest last. Device work: k_lag_slide, then 3 (I +
 * 1) launches, the C frame copies and one copy of the results (which also
 * brings back T_p and Cov_p). record = 1: mantis_get_smooth_record / _pass
 * serve the last push as window 0.
 *
 * MANTIS_ERR_ARG (nothing launched, the window unchanged, mantis_last_error
 * names the field): push before reset, no map, capacity or cams_per_rig out of
 * range, a smoothing parameter outside its range, a frame size differing from
 * the first push, a pose or motion that is not finite, a missing T_start where
 * it is required, a missing motion after the first push, a null pointer. */
typedef struct mantis_lag_params {
  int32_t struct_size;     /* sizeof(mantis_lag_params) */
  int32_t capacity;        /* N, 2..256 */
  int32_t cams_per_rig;    /* C, 1..8 */
  int32_t pad;
  mantis_smooth_params smooth;
} mantis_lag_params;
/* capacity 8, one camera, mantis_default_smooth_params */
void mantis_default_lag_params(mantis_lag_params* p);

typedef struct mantis_lag_info {
  int64_t pushes;          /* since the reset, this one included */
  int64_t oldest_stamp_ns; /* cams[0].stamp_ns of the oldest view held */
  int32_t n_views;         /* views held */
  int32_t has_prior;       /* this push's solve carried a prior */
  int32_t drop_reason;     /* 0, or why this push's slide left no prior (above) */
  int32_t slid;            /* this push marginalised a view out */
} mantis_lag_info;
/* sizeof(mantis_lag_params), sizeof(mantis_lag_info) (host only) */
void mantis_lag_sizes(int32_t* params_bytes, int32_t* info_bytes);

mantis_status mantis_lag_reset(void* ctx, const mantis_lag_params* p, const double* prior_T, const double* prior_cov);
mantis_status mantis_lag_push(void* ctx, const mantis_image* cams, const mantis_motion* motion, const double* T_start,
                              mantis_smooth_result* out_result, mantis_smooth_view* out_views,
                              mantis_lag_info* out_info /* nullable */);
/* The prior the next push's solve will use (T 16, cov 36, *has 0 / 1; each
 * nullable): the reset's or the carried one while the window is not full; once
 * it is full, the marginal of the oldest view held, computed now as the next
 * push will compute it (one small launch). *reason (nullable): drop_reason. */
mantis_status mantis_lag_get_prior(void* ctx, double* T, double* cov, int32_t* has, int32_t* reason);
/* The last push's views again. *n: in, the entries `views` has room for; out,
 * the views held. MANTIS_ERR_ARG when there is too little room. */
mantis_status mantis_lag_get_views(void* ctx, mantis_smooth_view* views, int32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* MANTIS_H */
