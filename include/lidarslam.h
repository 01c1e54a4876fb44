/*
 * lidarslam.h — C ABI of the MI355X-native per-scan hot path of
 * Farofeiro231/LiDAR_SLAM (RANSAC line/landmark extraction + UKF step).
 *
 * Plain pointers and sizes only; no torch, no C++ types.  Every function
 * returns an int status (LSLAM_OK = 0, < 0 on error) and never aborts.
 * Device pointers are HIP device memory (lslam_malloc or any hipMalloc'd
 * buffer); work is enqueued on the context's own HIP streams and is
 * asynchronous unless stated otherwise (lslam_sync waits for all of them).
 * lslam_h2d / lslam_d2h / lslam_memset are ordered after every earlier call
 * on the context (a pipeline call may finish on a side stream).
 *
 * Reference interfaces each entry point replaces (reference = /root/reference,
 * fit.py = scikit-image 0.18.3 skimage/measure/fit.py, the third-party code the
 * reference calls):
 *   lslam_polar_to_xy     functions.py:59-60   (dX, dY of each measure)
 *   lslam_express_decode  lidar.py:55-91 ExpressPacket.decode + :179-187
 *                         _process_express_scan over the :327-338 measure stream
 *   lslam_express_scans   the above + functions.py:56-76 (A1 + the A2 chunking of
 *                         each revolution fed to rawPoints)
 *   lslam_hyp_mt19937     fit.py:819-826 random_state.choice(N, 2, replace=False)
 *                         on the global np.random legacy MT19937 stream
 *   lslam_ransac          ransac_functions.py:23-31  ransac(data, LineModelND, 2, 20,
 *                         max_trials=100) + a, b, tip (fit.py:581-881, 19-132)
 *   lslam_landmarks       ransac_functions.py:34-54 association walk +
 *                         landmarking.py:48-77 + check_ransac append (:75-76)
 *   lslam_scan_pipeline   ransac_functions.py:63-93 check_ransac over the chunks
 *                         of many scans (landmark_extraction per chunk), fused with
 *                         the UKF step below
 *   lslam_ukf_step        systemClass.py:12-29 System.ukf.predict(u=..) +
 *                         .update(z, landmarks=..) with UKFMethods.py:10-71
 *                         callbacks (filterpy 1.4.5 UnscentedKalmanFilter semantics)
 *   lslam_ukf_trace       the same, exposing UKFMethods.py:26-34 hx and :60-71
 *                         residuals for the reference-pinned tests
 *   lslam_scan_match      nothing: the reference's robot.py holds a pose and no odometry; this is
 *                         the wheel-speed input u of UKFMethods.py:17-24 made from the scans
 *   lslam_grid_update     nothing persistent: mainWindow.py draws the last revolution's points
 *                         (allSeries.replace) and forgets them; this keeps a log-odds map of them
 *   lslam_map_match       nothing: the reference never reads a map back; this localises a revolution in
 *                         the log-odds grid, the absolute correction that the grid makes possible
 *   lslam_map_relocalize  nothing: the same, without a pose guess (a restart in a stored grid)
 */
#ifndef LIDARSLAM_H
#define LIDARSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSLAM_ABI_VERSION 6

/* ---- status codes ---- */
enum {
    LSLAM_OK = 0,
    LSLAM_ERR_ARG = -1,         /* invalid argument (ValueError in the reference) */
    LSLAM_ERR_HIP = -2,         /* HIP runtime error (message: lslam_last_error) */
    LSLAM_ERR_NOMEM = -3,
    LSLAM_ERR_CAPACITY = -4,    /* a landmark list or chunk count exceeded its capacity */
    LSLAM_ERR_UNSUPPORTED = -5  /* e.g. min_samples != 2 */
};

/* ---- per-chunk flags (lslam_chunk_model.flags) ---- */
enum {
    LSLAM_VALID = 1,          /* model fitted; landmark_extraction returned normally */
    LSLAM_N_TOO_SMALL = 2,    /* N < 3: fit.py:798-799 ValueError, no RNG consumed */
    LSLAM_NO_INLIERS = 4,     /* fit.py:877-879 (None, None) -> AttributeError at ransac_functions.py:25 */
    LSLAM_EST_FAIL = 8,       /* 1 final inlier: fit.py:96-97 ValueError */
    LSLAM_EARLY_STOP = 16,    /* stop_residuals_sum hit (sum of squared residuals == 0) */
    LSLAM_VERTICAL = 32,      /* final direction x == 0: a = +-inf/nan (ransac_functions.py:26) */
    LSLAM_NEW_LANDMARK = 64,  /* no landmark matched: the chunk's Landmark was appended */
    LSLAM_MATCHED = 128,      /* an existing landmark matched (its life reset to LIFE) */
    LSLAM_CAPACITY = 256,     /* no match and the list was full: the new landmark was dropped */
    LSLAM_CHUNK_BOUND = 512   /* LSLAM_UKF_MAP only: a matched chunk at index >= max_scan_chunks of its
                                 scan (an understated max_scan_chunks) has no measurement slot, so the
                                 UKF update does not use it; association and outputs are unaffected */
};

/* ---- hypothesis sources ---- */
enum {
    LSLAM_HYP_MT19937 = 0,  /* numpy legacy RandomState stream, bit-exact with the reference */
    LSLAM_HYP_PHILOX = 1,   /* counter-based Philox4x32-10, statistically equivalent only */
    LSLAM_HYP_EXPLICIT = 2  /* caller-provided draws (lslam_scan_batch.hyp) */
};

/* ---- UKF flags ---- */
enum {
    LSLAM_UKF_PREDICT = 1,
    LSLAM_UKF_UPDATE = 2,
    LSLAM_UKF_LMK_FROM_RANSAC = 4, /* landmark slot c <- chunk c's Landmark.pos (fused pipeline) */
    /* Landmark MAP mode (lslam_scan_pipeline with landmarks only): each scan's
     * landmark list is a persistent WORLD-frame map.  Per scan: predict (if PREDICT); every fitted
     * chunk line (ransac_functions.py:25-31, robot frame) is moved into the world frame by the
     * predicted pose x = [tx, ty, th] (p_w = R(th) p + t; a, b from the rotated direction); the
     * association walk (ransac_functions.py:34-54) runs on the map; each chunk that MATCHED a map
     * landmark j becomes one range/bearing measurement against hx(x, pos_j) (UKFMethods.py:26-34):
     * z_c = [|f|, atan2(f_y, f_x)], f = the foot of pos_j (moved into the robot frame by the
     * predicted pose) on the chunk's fitted line (is_equal matches any segment continuing the same
     * wall, so the chunk's own origin is not pos_j's re-observation); update (if UPDATE and >= 1
     * match) with those measurements only.  ukf_z / ukf_lmk are not read; n_landmarks = measurement slots, one per
     * chunk of a scan (>= max_scan_chunks); R_diag[2c], R_diag[2c+1] is slot c's noise.
     * models[c] keeps the robot-frame fit; proj_a/proj_b (y_proj) stay the chunk's own line.
     * id_base (if given) is in/out in this mode: advanced by the scan's chunk count, as
     * check_ransac's landmarkNumber (ransac_functions.py:77), so steps chain without host syncs. */
    LSLAM_UKF_MAP = 8,
    /* lslam_ukf_step, an UPDATE without PREDICT in the same call: the sigma points are read from
     * lslam_scan_batch.ukf_sigmas (filterpy's self.sigmas_f, cached by the last predict) instead of
     * being drawn from (x, P); x and P are the current ones (filterpy UKF.update: cross_variance(self.x,
     * zp, self.sigmas_f, ...), self.P - K S K^T).  Not supported by lslam_scan_pipeline. */
    LSLAM_UKF_SIGMAS_IN = 16
};

/* One RANSAC call's result (one chunk), 112 bytes. */
typedef struct lslam_chunk_model {
    double ox, oy;          /* final model origin   (model_robust.params[0]) */
    double ux, uy;          /* final model direction (params[1]; sign arbitrary) */
    double a, b;            /* y = a*x + b         (ransac_functions.py:26-27) */
    double tip_x, tip_y;    /* Landmark.end        (ransac_functions.py:29-30) */
    double proj_a, proj_b;  /* line used for yBase: matched landmark's or own (:46,:49,:53) */
    int32_t n_inliers;      /* popcount of the inlier mask */
    int32_t best_trial;     /* winning hypothesis index (-1 if none) */
    int32_t n_draws;        /* choice() draws consumed: T+1, or stop_trial+2 on early stop */
    int32_t flags;          /* LSLAM_* flags above */
    int32_t match_index;    /* index of the matched landmark in the pre-call list, -1 if none */
    int32_t landmark_id;    /* landmarkNumber given to this chunk's Landmark */
    int32_t n_points;       /* chunk size N */
    int32_t reserved;
} lslam_chunk_model;

/* landmarking.Landmark (landmarking.py:12-19), 56 bytes. */
typedef struct lslam_landmark {
    double a, b;
    double pos_x, pos_y;   /* Landmark.pos = final model origin */
    double end_x, end_y;   /* Landmark.end = (tipX, tipY) */
    int32_t id;
    int32_t life;
} lslam_landmark;

typedef struct lslam_ransac_params {
    double residual_threshold;  /* ransac_functions.py:9  THRESHOLD = 20 */
    int32_t max_trials;         /* ransac_functions.py:10 MAX_TRIALS = 100 */
    int32_t min_samples;        /* ransac_functions.py:11 MIN_SAMPLES = 2 (only 2 supported) */
    int32_t hyp_source;         /* LSLAM_HYP_* */
    int32_t life;               /* landmarking.py:3 LIFE = 40 */
    double tol_a;               /* landmarking.py:4 TOLERANCE_A = 0.1 */
    double tol_b;               /* landmarking.py:5 TOLERANCE_B = 10 */
    double tol_dist;            /* landmarking.py:6 TOLERANCE = 100 */
    uint64_t philox_seed;       /* LSLAM_HYP_PHILOX key */
} lslam_ransac_params;

typedef struct lslam_ukf_params {
    int32_t n_landmarks;     /* L; dim_z = 2L (systemClass.py:7 LANDMARK_NUMBER = 8) */
    int32_t flags;           /* LSLAM_UKF_* */
    double dt;               /* systemClass.py:10 DT = 0.005 */
    double wheel_radius;     /* UKFMethods.py:6 R = 50 (mm) */
    double wheel_base;       /* UKFMethods.py:7 L = 200 (mm) */
    double alpha, beta, kappa; /* systemClass.py:20 MerweScaledSigmaPoints(3, 1e-4, 2, 0) */
    double Q[9];             /* systemClass.py:29 Q = 1e-3 * I3 */
} lslam_ukf_params;

/* A batch of scans, all pointers DEVICE memory (NULL = absent where optional). */
typedef struct lslam_scan_batch {
    int32_t n_scans;
    int32_t n_chunks;               /* = scan_chunk_off[n_scans] */
    int64_t n_points;               /* = chunk_pt_off[n_chunks] */
    int32_t max_chunk_points;       /* max chunk size N over the batch */
    int32_t max_scan_chunks;        /* max chunks per scan: sizes the post pass's LDS staging.  A scan with
                                       more chunks gets the same results through the unstaged paths (a
                                       rewind snapshot per chunk, records walked in place); only
                                       LSLAM_UKF_MAP's measurement slots stop there (LSLAM_CHUNK_BOUND) */
    int32_t lmk_capacity;           /* per-scan landmark list capacity */
    int32_t reserved;
    /* inputs */
    const double *xy;               /* [n_points][2] fp64 Cartesian points (AoS); NULL: theta_deg / dist_mm */
    const int32_t *scan_chunk_off;  /* [n_scans+1] CSR scan -> chunks */
    const int32_t *chunk_pt_off;    /* [n_chunks+1] CSR chunk -> points */
    const uint32_t *seeds;          /* [n_scans] np.random.seed(seed) per scan (MT19937 mode) */
    const uint32_t *mt_state_in;    /* [n_scans][625] key[624] + pos, overrides seeds */
    uint32_t *mt_state_out;         /* [n_scans][625] state after the scan (optional) */
    const int32_t *hyp;             /* [n_chunks][max_trials+1][2] (LSLAM_HYP_EXPLICIT) */
    const int32_t *id_base;         /* [n_scans] landmarkNumber of the first chunk (optional, 0) */
    lslam_landmark *landmarks;      /* [n_scans][lmk_capacity] in/out (optional) */
    int32_t *lmk_count;             /* [n_scans] in/out (required with landmarks) */
    int32_t *lmk_walk;              /* [n_scans][lmk_capacity] out (optional): life of each entry of the
                                       list as it was before the scan's LAST chunk, after that chunk's
                                       association walk (0 = removed); lets a caller holding its own
                                       list objects apply the walk (the drop-in shim) */
    /* outputs */
    uint8_t *inlier_mask;           /* [n_points] */
    lslam_chunk_model *models;      /* [n_chunks] */
    double *y_proj;                 /* [n_points] projected y of inliers, 0 elsewhere (optional) */
    int32_t *draws_out;             /* [n_chunks][max_trials+1][2] (optional, parity/debug) */
    int32_t *trial_cnt_out;         /* [n_chunks][max_trials] (optional, parity/debug; zero rows
                                       for chunks of fewer than 3 points) */
    /* UKF, per scan */
    double *ukf_x;                  /* [n_scans][3] in/out */
    double *ukf_P;                  /* [n_scans][3][3] in/out */
    const double *ukf_u;            /* [n_scans][2]  [vl, vr] */
    const double *ukf_z;            /* [n_scans][2L] interleaved [d0, phi0, d1, phi1, ...] (not in MAP mode) */
    const double *ukf_lmk;          /* [n_scans][L][2] landmark positions (not in MAP mode) */
    const double *ukf_R_diag;       /* [2L] measurement noise diagonal (systemClass.py:28) */
    /* A1 fused into the point loads (ABI 2): with xy == NULL the points are
     * the raw measures and every kernel that reads a point converts it as functions.py:59-60 does,
     * x = d cos(-th * pi/180 + pi/2), y = d sin(...), bit-identical to lslam_polar_to_xy. */
    const double *theta_deg;        /* [n_points] */
    const double *dist_mm;          /* [n_points] */
    /* ABI 4: filterpy's sigmas_f per scan, [n_scans][7][3] (optional; lslam_ukf_step only): a PREDICT
     * writes the sigma points re-drawn from the predicted (x, P); an UPDATE with LSLAM_UKF_SIGMAS_IN
     * reads them.  NULL: not written, and an update draws its sigma points from (x, P). */
    double *ukf_sigmas;
} lslam_scan_batch;

/* Express-scan measures (lslam_express_decode): device arrays, NULL = not written.
 * Packet p (< M-1) yields measures 32p .. 32p+31 (trame 1..32, using packet p+1's start angle). */
typedef struct lslam_express_measures {
    double *angle_deg;    /* [(M-1)*32] lidar.py:185 (0 where invalid) */
    double *dist_mm;      /* [(M-1)*32] ExpressPacket.distance (0 where invalid) */
    uint8_t *new_scan;    /* [(M-1)*32] lidar.py:181-184 */
    uint8_t *valid;       /* [(M-1)*32] packets p and p+1 both decode */
    double *xy;           /* [(M-1)*32][2] functions.py:59-60 (A1 fused) */
    uint8_t *pkt_valid;   /* [M] ExpressPacket.decode would not raise */
} lslam_express_measures;

/* Express-scan revolutions (lslam_express_scans): device arrays sized by the caller.
 * Safe capacities for M packets: cap_points = 32(M-1), cap_scans = M-1,
 * cap_chunks = 32(M-1)/100 + M-1.  counts (device, int32[4]) receives
 * n_scans, n_chunks, n_points, and the packet holding the last new-revolution
 * flag (-1 if none): resume the stream from that packet with skip = 1. */
typedef struct lslam_express_revs {
    double *xy;                 /* [cap_points][2] */
    int32_t *scan_chunk_off;    /* [cap_scans + 1] CSR revolution -> chunks */
    int32_t *chunk_pt_off;      /* [cap_chunks + 1] CSR chunk -> points */
    int32_t *counts;            /* [4] */
    int64_t cap_points;
    int32_t cap_scans, cap_chunks;
} lslam_express_revs;

/* ---- scan-match flags (lslam_match_batch.flags) ---- */
enum {
    LSLAM_MATCH_EMPTY = 1,  /* no valid point on one side, or a winning score of 0: delta = 0, best = the centre */
    LSLAM_MATCH_EDGE = 2    /* the winner lies on the window's border along some axis: the motion may exceed it */
};

/* Correlative scan matcher (lslam_scan_match).  Ranges: cell > 0, theta_step > 0, grid_w even in
 * 16..512, smear 0..2, k_trans 0..15, k_theta 0..31. */
typedef struct lslam_match_params {
    double cell;        /* cell size, mm (20) */
    double theta_step;  /* rotation step, rad (pi/360) */
    int32_t grid_w;     /* cells per side of the look-up grid (512) */
    int32_t smear;      /* smear radius, cells (2) */
    int32_t k_trans;    /* translation half-window, cells (10): Nt = 2 k_trans + 1 */
    int32_t k_theta;    /* rotation half-window, steps (20): Ntheta = 2 k_theta + 1 */
} lslam_match_params;

/* A batch of scan pairs, one per robot; all pointers DEVICE memory (NULL = absent where optional). */
typedef struct lslam_match_batch {
    int32_t n_scans;
    int32_t reserved;
    /* inputs */
    const double *ref_xy;    /* [ref_off[n_scans]][2] previous revolutions, each in its own robot frame */
    const int32_t *ref_off;  /* [n_scans+1] CSR robot -> reference points */
    const double *cur_xy;    /* [cur_off[n_scans]][2] current revolutions */
    const int32_t *cur_off;  /* [n_scans+1] */
    const double *rot;       /* [Ntheta][2] (cos, sin) of (k - k_theta) * theta_step: the caller's bits */
    /* outputs */
    double *delta;           /* [n_scans][3] (tx mm, ty mm, dtheta rad): current frame in the previous one */
    int32_t *best;           /* [n_scans][4] (k, jy, jx, score) of the winner */
    int32_t *n_valid;        /* [n_scans][2] valid reference / current points */
    int32_t *flags;          /* [n_scans] LSLAM_MATCH_* */
    int32_t *scores;         /* [n_scans][Ntheta][Nt][Nt] the whole score volume (optional) */
    double *ukf_u;           /* [n_scans][2] wheel speeds [vl, vr] (optional; written only with u != NULL) */
} lslam_match_batch;

/* ---- occupancy-grid flags (lslam_grid_batch.flags) ---- */
enum {
    LSLAM_GRID_BAD_POSE = 1,  /* a non-finite pose or origin, or a robot cell 2^20 or more cells off: grid untouched */
    LSLAM_GRID_CLIPPED = 2    /* some cell of some ray lies outside the grid */
};

/* Occupancy-grid mapping (lslam_grid_update), 40 bytes.  Ranges: cell > 0; max_range > 0, finite,
 * max_range / cell <= 4096; grid_w 16..2048; l_hit 1..1024; l_miss -1024..-1;
 * -32768 <= l_min < 0 < l_max <= 32767. */
typedef struct lslam_grid_params {
    double cell;       /* cell size, mm (20) */
    double max_range;  /* returns farther than this are ignored, mm (8000) */
    int32_t grid_w;    /* cells per side (512) */
    int32_t l_hit;     /* log-odds of a hit, 0.01 nat (85: p = 0.7) */
    int32_t l_miss;    /* log-odds of a pass, 0.01 nat (-41: p = 0.4) */
    int32_t l_min;     /* clamp (-200: p ~ 0.12) */
    int32_t l_max;     /* clamp (350: p ~ 0.97) */
    int32_t reserved;
} lslam_grid_params;

/* One revolution per robot, 72 bytes; all pointers DEVICE memory, all required. */
typedef struct lslam_grid_batch {
    int32_t n_robots;
    int32_t reserved;
    /* inputs */
    const double *xy;       /* [pt_off[n_robots]][2] revolutions, each in its robot's frame */
    const int32_t *pt_off;  /* [n_robots+1] CSR robot -> points */
    const double *pose;     /* [n_robots][3] (x mm, y mm, theta rad), e.g. the filter's ukf_x */
    const double *origin;   /* [n_robots][2] world coordinates of the corner of cell (0, 0) */
    /* in/out */
    int16_t *logodds;       /* [n_robots][grid_w][grid_w], row Y, units of 0.01 nat */
    /* outputs */
    double *rot;            /* [n_robots][2] (cos theta, sin theta) as used */
    int32_t *n_used;        /* [n_robots][2] points traced / valid points beyond max_range */
    int32_t *flags;         /* [n_robots] LSLAM_GRID_* */
} lslam_grid_batch;

/* ---- scan-to-map flags (lslam_mapmatch_batch.flags) ---- */
enum {
    LSLAM_MAPMATCH_EMPTY = 1,     /* a winning score of 0 (no valid point on an occupied cell): delta = 0, best = the centre */
    LSLAM_MAPMATCH_EDGE = 2,      /* the winner lies on the search window's border along some axis */
    LSLAM_MAPMATCH_BAD_POSE = 4,  /* as LSLAM_GRID_BAD_POSE: nothing is matched */
    LSLAM_MAPMATCH_WEAK = 8,      /* the winner's score is below the acceptance gate: pose_out = pose */
    /* lslam_map_fuse only, in the same word: */
    LSLAM_MAPFUSE_OUTLIER = 16,   /* the innovation's Mahalanobis distance exceeds nis_max: no update */
    LSLAM_MAPFUSE_BAD_COV = 32    /* P is not finite, or P + Rm is not positive definite: no update, nis = 0 */
};

/* Scan-to-map matcher (lslam_map_match), 32 bytes.  The cell size and the map's width come from the
 * lslam_grid_params given with the call. */
typedef struct lslam_mapmatch_params {
    double theta_step;    /* rotation step, rad (pi/360); > 0, finite */
    int32_t win_w;        /* cells per side of the look-up window, even, 16..512 (512) */
    int32_t smear;        /* smear radius, cells, 0..2 (2) */
    int32_t k_trans;      /* translation half-window, cells, 0..15 (10): Nt = 2 k_trans + 1 */
    int32_t k_theta;      /* rotation half-window, steps, 0..31 (20): Ntheta = 2 k_theta + 1 */
    int32_t occ_min;      /* a map cell is occupied iff L >= occ_min; -32768..32767 (85: one hit) */
    int32_t min_permille; /* acceptance gate, 0..1000 (500) */
} lslam_mapmatch_params;

/* One revolution per robot against the robot's grid, 112 bytes; all pointers DEVICE memory, all
 * required but scores. */
typedef struct lslam_mapmatch_batch {
    int32_t n_robots;
    int32_t reserved;
    /* inputs */
    const double *xy;         /* [pt_off[n_robots]][2] revolutions, each in its robot's frame */
    const int32_t *pt_off;    /* [n_robots+1] CSR robot -> points */
    const double *pose;       /* [n_robots][3] the guess (x mm, y mm, theta rad), e.g. the filter's ukf_x */
    const double *origin;     /* [n_robots][2] world coordinates of the corner of cell (0, 0) */
    const int16_t *logodds;   /* [n_robots][grid_w][grid_w], row Y: read only */
    const double *rot;        /* [Ntheta][2] (cos, sin) of (k - k_theta) * theta_step: the caller's bits */
    /* outputs */
    double *pose_out;         /* [n_robots][3] the corrected pose, or the guess bit for bit; MAY ALIAS pose */
    double *delta;            /* [n_robots][3] world-frame correction (dx mm, dy mm, dtheta rad) */
    int32_t *best;            /* [n_robots][4] (k, jy, jx, score) of the winner */
    int32_t *n_valid;         /* [n_robots][2] occupied cells in the window / valid points */
    double *rot0;             /* [n_robots][2] (cos theta, sin theta) of the guess, as used */
    int32_t *flags;           /* [n_robots] LSLAM_MAPMATCH_* */
    int32_t *scores;          /* [n_robots][Ntheta][Nt][Nt] the whole score volume (optional) */
} lslam_mapmatch_batch;

/* Match fusion (lslam_map_fuse), 24 bytes. */
typedef struct lslam_mapfuse_params {
    double r_scale;        /* factor on the match covariance Rm; finite, > 0 (1.0) */
    double nis_max;        /* gate on the innovation's Mahalanobis distance; > 0, +inf: no gate (16.27: the
                              99.9 % point of chi-square with 3 degrees of freedom) */
    int32_t cut_permille;  /* candidates scoring above cut_permille / 1000 of the winner weigh in; 0..999 (900) */
    int32_t reserved;
} lslam_mapfuse_params;

/* A scan-to-map match fused into the filter, 160 bytes: the match's batch with its fields and rules
 * as they are (m.pose is the filter's mean and the search's guess, m.pose_out the updated mean,
 * m.scores stays optional), then the covariance and the measurement; all pointers DEVICE memory, all
 * required but m.scores and moments. */
typedef struct lslam_mapfuse_batch {
    lslam_mapmatch_batch m;
    const double *P;          /* [n_robots][9] the filter's covariance, row-major, e.g. ukf_P */
    double *P_out;            /* [n_robots][9] the updated covariance, or P bit for bit; MAY ALIAS P */
    double *z;                /* [n_robots][3] the match as a measurement of the pose: pose + delta */
    double *Rm;               /* [n_robots][9] its covariance, row-major */
    double *nis;              /* [n_robots] the innovation's squared Mahalanobis distance */
    int64_t *moments;         /* [n_robots][10] the integer moments of the score volume (optional) */
} lslam_mapfuse_batch;

/* ---- relocalisation flags (lslam_reloc_batch.flags) ---- */
enum {
    LSLAM_RELOC_LOST = 1,       /* no candidate passed the fine matcher's gates: pose_out untouched */
    LSLAM_RELOC_AMBIGUOUS = 2   /* a second, distinct pose scores within ambig_permille of the winner: pose_out untouched */
};

/* Global relocalisation (lslam_map_relocalize), 56 bytes. */
typedef struct lslam_reloc_params {
    double head_step;          /* heading step of the coarse search, rad (2 pi / 180); > 0, finite */
    double dup_mm;             /* two refined poses this close along x and y ... ; >= 0 (100.0) */
    double dup_rad;            /* ... and in heading are one pose; >= 0 (0.0873) */
    double reset_sigma_xy;     /* P_out of a found robot: diag(sxy^2, sxy^2, sth^2); > 0, finite (50.0 mm) */
    double reset_sigma_theta;  /* > 0, finite (0.05 rad) */
    int32_t n_head;            /* headings of the coarse search, 4..1024 (180) */
    int32_t factor;            /* fine cells per coarse cell and side: 2, 4 or 8, a divisor of grid_w with
                                  grid_w / factor in 4..256 (4) */
    int32_t n_cand;            /* K, coarse peaks refined by the fine matcher, 1..16 (8) */
    int32_t ambig_permille;    /* a rival at this share of the winner's fine score is an ambiguity, 0..1000 (900) */
} lslam_reloc_params;

/* One revolution per robot against the robot's grid, no pose guess, 176 bytes; all pointers DEVICE
 * memory, all required but P_out and coarse_scores.  K = n_cand, Wc = grid_w / factor. */
typedef struct lslam_reloc_batch {
    int32_t n_robots;
    int32_t reserved;
    /* inputs */
    const double *xy;         /* [pt_off[n_robots]][2] revolutions, each in its robot's frame */
    const int32_t *pt_off;    /* [n_robots+1] CSR robot -> points */
    const double *origin;     /* [n_robots][2] world coordinates of the corner of cell (0, 0) */
    const int16_t *logodds;   /* [n_robots][grid_w][grid_w], row Y: read only */
    const double *rot;        /* [Ntheta][2] the fine matcher's table, as lslam_mapmatch_batch.rot */
    const double *head_rot;   /* [n_head][2] (cos, sin) of k * head_step: the caller's bits */
    /* outputs */
    int32_t *n_occ;           /* [n_robots] occupied coarse cells */
    int32_t *n_used;          /* [n_robots] valid points within max_range */
    int32_t *cand;            /* [K][n_robots][4] (k, ty, tx, coarse score) of rank j; (-1, -1, -1, 0) if missing */
    double *cand_pose;        /* [K][n_robots][3] the pose of rank j's coarse cell; quiet NaNs if missing */
    double *fine_pose;        /* [K][n_robots][3] lslam_map_match's pose_out from cand_pose[j] */
    double *fine_delta;       /* [K][n_robots][3] its delta */
    int32_t *fine_best;       /* [K][n_robots][4] its best */
    int32_t *fine_nvalid;     /* [K][n_robots][2] its n_valid */
    double *fine_rot0;        /* [K][n_robots][2] its rot0 */
    int32_t *fine_flags;      /* [K][n_robots] its flags */
    int32_t *result;          /* [n_robots][8] winner rank, its k, ty, tx, coarse score, fine score, best rival's
                                 rank or -1, that rival's fine score or 0 */
    int32_t *flags;           /* [n_robots] LSLAM_RELOC_* */
    double *pose_out;         /* [n_robots][3] written for a found, unambiguous robot only, e.g. ukf_x */
    double *P_out;            /* [n_robots][9] the same (optional), e.g. ukf_P */
    int32_t *coarse_scores;   /* [n_robots][n_head][Wc][Wc] the whole coarse volume (optional) */
} lslam_reloc_batch;

/* Relocalisation priors (lslam_map_relocalize_prior), 24 bytes. */
typedef struct lslam_relocprior_params {
    double half_xy;      /* mm, >= 0, +inf: no box; half side of the window box around win_pose (x, y) (1000.0) */
    double half_theta;   /* rad, >= 0, +inf: every heading (0.5) */
    int32_t clear_min2;  /* squared fine cells, 0..65025 (16: four cells, one default coarse cell) */
    int32_t reserved;
} lslam_relocprior_params;

/* lslam_reloc_batch with the priors and their two outputs, 208 bytes; all pointers DEVICE memory,
 * clear_d2 and win_pose optional, n_admit and fine_clear2 required. */
typedef struct lslam_relocprior_batch {
    lslam_reloc_batch r;       /* as it is, every rule of lslam_map_relocalize */
    const uint16_t *clear_d2;  /* [n_robots][grid_w][grid_w] the NOT_FREE field of lslam_grid_distance (optional) */
    const double *win_pose;    /* [n_robots][3] the centre of the search window, e.g. the stale ukf_x (optional) */
    int32_t *n_admit;          /* [n_robots][2] admissible coarse cells, admissible headings */
    int32_t *fine_clear2;      /* [K][n_robots] d2 at the refined pose's cell; -1 off the map or rank missing;
                                  0 if clear_d2 is NULL */
} lslam_relocprior_batch;

/* ---- grid ray-cast flags (lslam_raycast_batch.flags), beam classes and stop kinds (cls) ---- */
enum {
    LSLAM_RAYCAST_BAD_POSE = 1  /* as LSLAM_GRID_BAD_POSE: nothing is cast */
};
enum {
    LSLAM_RAYCAST_INVALID = 0,   /* not a valid point (or a denormal one): nothing is cast */
    LSLAM_RAYCAST_MATCH = 1,     /* the beam returned where the map says it stops */
    LSLAM_RAYCAST_NOVEL = 2,     /* a return inside space the map holds free: a dynamic object */
    LSLAM_RAYCAST_THROUGH = 3,   /* the beam passed a cell the map holds occupied: a stale map or a wrong pose */
    LSLAM_RAYCAST_UNMAPPED = 4   /* the beam ran into unknown space at or before its return */
};
enum {
    LSLAM_RAYCAST_KIND_NONE = 0,     /* the ray left the range circle still free */
    LSLAM_RAYCAST_KIND_UNKNOWN = 1,  /* it stopped at an unknown cell, or off the map */
    LSLAM_RAYCAST_KIND_OCC = 2       /* it stopped at an occupied cell */
};

/* Grid ray casting (lslam_grid_raycast), 16 bytes.  The grid's geometry comes from the
 * lslam_grid_params given with the call. */
typedef struct lslam_raycast_params {
    int32_t occ_min;   /* a cell is occupied iff L >= occ_min; -32768..32767 (1: more hits than passes, p > 0.5) */
    int32_t free_max;  /* a cell is free iff L <= free_max; -32768..32766 and < occ_min (-1: p < 0.5; L = 0 alone
                          is unknown.  The matchers' 85 and one pass's -41 leave the cells beside a wall,
                          one hit and a few passes, unknown: DESIGN.md 4.4) */
    int32_t tol;       /* tolerance in steps along the ray, 0..64 (3) */
    int32_t reserved;
} lslam_raycast_params;

/* One revolution per robot cast through the robot's grid, 88 bytes; all pointers DEVICE memory, all
 * required but stop.  P = pt_off[n_robots]. */
typedef struct lslam_raycast_batch {
    int32_t n_robots;
    int32_t reserved;
    /* inputs */
    const double *xy;         /* [P][2] revolutions, each in its robot's frame */
    const int32_t *pt_off;    /* [n_robots+1] CSR robot -> points */
    const double *pose;       /* [n_robots][3] (x mm, y mm, theta rad), e.g. the filter's ukf_x */
    const double *origin;     /* [n_robots][2] world coordinates of the corner of cell (0, 0) */
    const int16_t *logodds;   /* [n_robots][grid_w][grid_w], row Y: read only */
    /* outputs */
    uint8_t *cls;             /* [P] class | kind << 4 */
    int32_t *stop;            /* [P][3] (ox, oy, i_h): where the map stops the beam, in cells from the robot cell (optional) */
    int32_t *counts;          /* [n_robots][8] points of classes 0..4, valid points beyond max_range, points of kind NONE, 0 */
    double *rot;              /* [n_robots][2] (cos theta, sin theta) as used */
    int32_t *flags;           /* [n_robots] LSLAM_RAYCAST_* */
} lslam_raycast_batch;

/* ---- grid recentre flags (lslam_recentre_batch.flags) ---- */
enum {
    LSLAM_RECENTRE_BAD_POSE = 1,  /* as LSLAM_GRID_BAD_POSE, or a new origin that is not finite: nothing moves */
    LSLAM_RECENTRE_MOVED = 2,     /* the grid and its origin were shifted by shift[r] cells */
    LSLAM_RECENTRE_CLEARED = 4    /* with MOVED: the shift is a whole map or more on an axis, nothing was kept */
};

/* Grid recentre (lslam_grid_recentre), 16 bytes.  The grid's geometry comes from the lslam_grid_params
 * given with the call. */
typedef struct lslam_recentre_params {
    int32_t margin;    /* cells: the robot cell may come this near an edge before the grid moves; 0..grid_w/2 (128) */
    int32_t quantum;   /* cells: shifts are multiples of it; 1..64 (8: a moved row stays on the 16-byte groups
                          that the readers load) */
    int32_t reserved[2];
} lslam_recentre_params;

/* One recentre per robot, 48 bytes; all pointers DEVICE memory, all required. */
typedef struct lslam_recentre_batch {
    int32_t n_robots;
    int32_t reserved;
    const double *pose;       /* [n_robots][3] (x mm, y mm, theta rad), e.g. the filter's ukf_x */
    double *origin;           /* [n_robots][2] in/out: world coordinates of the corner of cell (0, 0) */
    int16_t *logodds;         /* [n_robots][grid_w][grid_w] in/out, row Y */
    int32_t *shift;           /* [n_robots][2] (sx, sy) in cells: the grid now starts that many cells further on */
    int32_t *flags;           /* [n_robots] LSLAM_RECENTRE_* */
} lslam_recentre_batch;

/* ---- page flags (lslam_page_batch.flags) ---- */
enum {
    LSLAM_PAGE_LOST = 1       /* cells that left the window were off the canvas: they are gone */
};

/* The paged rolling grid (lslam_grid_recentre_paged, lslam_grid_page_flush, lslam_grid_page_load), 16 bytes. */
typedef struct lslam_page_params {
    int32_t canvas_w;         /* cells a side of every robot's canvas; 16..2048 (2048) */
    int32_t reserved[3];
} lslam_page_params;

/* One canvas per robot, 40 bytes; all pointers DEVICE memory.  flags is required by
 * lslam_grid_recentre_paged alone: flush and load neither read nor write it. */
typedef struct lslam_page_batch {
    int32_t n_robots;
    int32_t reserved;
    int16_t *canvas;          /* [n_robots][canvas_w][canvas_w] in/out, row Y */
    int32_t *win;             /* [n_robots][2] in/out (wx, wy): the canvas coordinates of window cell (0, 0) */
    int32_t *moved;           /* [n_robots][2] (cells stored to the canvas, cells loaded from it) */
    int32_t *flags;           /* [n_robots] LSLAM_PAGE_* */
} lslam_page_batch;

/* ---- distance-field modes (lslam_dist_params.mode) and flags (lslam_dist_batch.flags) ---- */
enum {
    LSLAM_DIST_OCC = 0,       /* the sources are the occupied cells: L >= occ_min */
    LSLAM_DIST_NOT_FREE = 1   /* the sources are the cells that are not free, L > free_max, and every cell off the map */
};
enum {
    LSLAM_DIST_EMPTY = 1      /* no source cell on the map */
};

/* Distance field (lslam_grid_distance), 16 bytes.  The grid's geometry is the grid_w of the
 * lslam_grid_params given with the call. */
typedef struct lslam_dist_params {
    int32_t mode;      /* LSLAM_DIST_OCC (0) or LSLAM_DIST_NOT_FREE */
    int32_t occ_min;   /* OCC: a cell is a source iff L >= occ_min; -32768..32767 (85, the matchers' threshold) */
    int32_t free_max;  /* NOT_FREE: a cell is a source iff L > free_max; -32768..32767 (-1, the ray caster's) */
    int32_t d_max;     /* cells, 1..255 (64): the field saturates at d_max^2 */
} lslam_dist_params;

/* One field per robot, 40 bytes; all pointers DEVICE memory, all required. */
typedef struct lslam_dist_batch {
    int32_t n_robots;
    int32_t reserved;
    const int16_t *logodds;   /* [n_robots][grid_w][grid_w], row Y: read only */
    uint16_t *d2;             /* [n_robots][grid_w][grid_w] out: min(squared distance in cells, d_max^2) */
    int32_t *n_src;           /* [n_robots] source cells on the map */
    int32_t *flags;           /* [n_robots] LSLAM_DIST_* */
} lslam_dist_batch;

/* ---- field-score flags (lslam_fieldscore_batch.flags) ---- */
enum {
    LSLAM_FIELD_BAD_POSE = 1  /* as LSLAM_GRID_BAD_POSE: nothing is scored */
};

/* The field read under a revolution (lslam_field_score), 16 bytes.  v is the field's value at a
 * point's hit cell. */
typedef struct lslam_fieldscore_params {
    int32_t trunc2;    /* a point adds min(v, trunc2); 1..65025 (625: 25 cells, an outlier costs no more) */
    int32_t near2;     /* a point is near iff v <= near2; 0..65025 (4) */
    int32_t off2;      /* v of a hit cell (or robot cell) off the map; 0..65025 (4096, the default d_max squared) */
    int32_t reserved;
} lslam_fieldscore_params;

/* One revolution per robot scored in the robot's field, 80 bytes; all pointers DEVICE memory, all
 * required.  P = pt_off[n_robots]. */
typedef struct lslam_fieldscore_batch {
    int32_t n_robots;
    int32_t reserved;
    /* inputs */
    const double *xy;         /* [P][2] revolutions, each in its robot's frame */
    const int32_t *pt_off;    /* [n_robots+1] CSR robot -> points */
    const double *pose;       /* [n_robots][3] (x mm, y mm, theta rad), e.g. the filter's ukf_x */
    const double *origin;     /* [n_robots][2] world coordinates of the corner of cell (0, 0) */
    const uint16_t *d2;       /* [n_robots][grid_w][grid_w] the field of lslam_grid_distance: read only */
    /* outputs */
    double *rot;              /* [n_robots][2] (cos theta, sin theta) as used */
    int64_t *stats;           /* [n_robots][4] (sum of min(v, trunc2), points scored, near points, points off the map) */
    int32_t *clear2;          /* [n_robots] d2 at the robot cell (off2 if it is off the map) */
    int32_t *flags;           /* [n_robots] LSLAM_FIELD_* */
} lslam_fieldscore_batch;

/* ---- field-align flags (lslam_fieldalign_batch.flags) ---- */
enum {
    LSLAM_FIELDALIGN_BAD_POSE = 1,   /* as LSLAM_GRID_BAD_POSE: nothing is evaluated, pose_out is pose */
    LSLAM_FIELDALIGN_CONVERGED = 2,  /* a step fell below eps_t and eps_r */
    LSLAM_FIELDALIGN_SINGULAR = 4,   /* a pivot of the solve is not finite and > 0, or the stepped pose is not finite: pose_out is pose */
    LSLAM_FIELDALIGN_FEW = 8,        /* an evaluation used fewer than min_points points: pose_out is pose */
    LSLAM_FIELDALIGN_DIVERGED = 16,  /* the pose left the guess by more than max_shift or max_turn: pose_out is pose */
    LSLAM_FIELDALIGN_WEAK = 32,      /* the last evaluation used less than min_permille of the valid points: pose_out is pose */
    /* lslam_field_fuse only, in the same word: */
    LSLAM_FIELDFUSE_OUTLIER = 64,    /* the innovation statistic exceeds nis_max: no update */
    LSLAM_FIELDFUSE_BAD_COV = 128    /* P is not finite, or one of the fusion's three inverses fails its test: no update, nis = 0 */
};

/* Gauss-Newton alignment in the distance field (lslam_field_align), 72 bytes.  Lengths in cells unless
 * said otherwise. */
typedef struct lslam_fieldalign_params {
    double trunc;      /* a point whose interpolated distance exceeds it is skipped; 0..255 (25.0, the square root
                          of lslam_fieldscore_params.trunc2) */
    double damp_t;     /* added to the two translation diagonals of J^T J; >= 0, finite (1.0) */
    double damp_r;     /* added to its rotation diagonal; >= 0, finite (100.0) */
    double eps_t;      /* cells: a step with max(|dx|, |dy|) below it ... */
    double eps_r;      /* ... and |dtheta| below this many rad has converged; both >= 0, finite (0.01, 1e-4) */
    double max_shift;  /* mm per axis: gate on the distance from the guess; >= 0, +inf: no gate (200.0) */
    double max_turn;   /* rad: the same for the heading; >= 0, +inf: no gate (0.1) */
    int32_t n_iter;        /* most steps, 1..32 (10) */
    int32_t min_points;    /* an evaluation needs this many used points; >= 0 (16) */
    int32_t min_permille;  /* gate on points used at the last evaluation / valid points, 0..1000 (500) */
    int32_t reserved;
} lslam_fieldalign_params;

/* One revolution per robot aligned in the robot's field, 96 bytes; all pointers DEVICE memory, all
 * required.  P = pt_off[n_robots], E = n_iter + 1. */
typedef struct lslam_fieldalign_batch {
    int32_t n_robots;
    int32_t reserved;
    /* inputs: as lslam_fieldscore_batch */
    const double *xy;         /* [P][2] revolutions, each in its robot's frame */
    const int32_t *pt_off;    /* [n_robots+1] CSR robot -> points */
    const double *pose;       /* [n_robots][3] the guess (x mm, y mm, theta rad), e.g. the filter's ukf_x */
    const double *origin;     /* [n_robots][2] world coordinates of the corner of cell (0, 0) */
    const uint16_t *d2;       /* [n_robots][grid_w][grid_w] the field of lslam_grid_distance: read only */
    /* outputs */
    double *pose_out;         /* [n_robots][3] the aligned pose, or pose bit for bit; may be pose itself */
    double *trace;            /* [n_robots][E][5] (px, py, theta, cos theta, sin theta) of every evaluation; zeros beyond the last */
    int64_t *normal;          /* [n_robots][10] the last evaluation's sums: J^T J (xx, xy, xt, yy, yt, tt), J^T r (x, y, t), r^2; times 2^20 */
    int32_t *n_used;          /* [n_robots][3] points used at the first evaluation, at the last, valid points within max_range */
    int32_t *iters;           /* [n_robots] steps taken */
    int32_t *flags;           /* [n_robots] LSLAM_FIELDALIGN_* */
} lslam_fieldalign_batch;

/* Field fusion (lslam_field_fuse), 48 bytes. */
typedef struct lslam_fieldfuse_params {
    double sigma_min;  /* floor on the residual standard deviation, cells; > 0, finite (0.5: the field resolves no less
                          than half a cell) */
    double r_scale;    /* factor on the noise variance; > 0, finite (1.0) */
    double floor_t;    /* covariance floor on x and y, as a standard deviation in cells; > 0, finite (1 / sqrt(12): one
                          cell's quantum, as lslam_map_fuse floors with one search quantum) */
    double floor_r;    /* the same for the heading, rad; > 0, finite ((pi / 360) / sqrt(12): the matcher's heading quantum) */
    double nis_max;    /* gate on the innovation statistic; > 0, +inf: no gate (16.27: the 99.9 % point of chi-square
                          with 3 degrees of freedom) */
    int64_t reserved;
} lslam_fieldfuse_params;

/* A field alignment fused into the filter, 152 bytes: the alignment's batch with its fields and rules as
 * they are (a.pose is the filter's mean and the guess, a.pose_out the UPDATED mean), then the covariance
 * and the measurement; all pointers DEVICE memory, all required. */
typedef struct lslam_fieldfuse_batch {
    lslam_fieldalign_batch a;
    const double *P;          /* [n_robots][9] the filter's covariance, row-major, e.g. ukf_P */
    double *P_out;            /* [n_robots][9] the updated covariance, or P bit for bit; MAY ALIAS P */
    double *z;                /* [n_robots][3] the aligned pose, or the guess bit for bit; overlaps none of a.pose,
                                 a.pose_out, P, P_out */
    double *info;             /* [n_robots][9] the alignment's information matrix, mm and rad, row-major */
    double *info_f;           /* [n_robots][9] the same with the covariance floor, the one that is fused */
    double *s2;               /* [n_robots] the noise variance, squared cells */
    double *nis;              /* [n_robots] the gated innovation statistic */
} lslam_fieldfuse_batch;

typedef struct lslam_ctx lslam_ctx;  /* opaque: device, stream, events, scratch */

/* ---- library / context ---- */
const char *lslam_version(void);
const char *lslam_status_string(int status);
const char *lslam_last_error(void);  /* thread-local message of the last error */
int lslam_device_count(int *n);
int lslam_ctx_create(int device, lslam_ctx **out);
int lslam_ctx_destroy(lslam_ctx *ctx);
int lslam_sync(lslam_ctx *ctx);
int lslam_malloc(lslam_ctx *ctx, size_t bytes, void **dptr);
int lslam_free(lslam_ctx *ctx, void *dptr);
int lslam_host_alloc(size_t bytes, void **hptr);  /* pinned host memory */
int lslam_host_free(void *hptr);
int lslam_h2d(lslam_ctx *ctx, void *dst, const void *src, size_t bytes);  /* async */
int lslam_d2h(lslam_ctx *ctx, void *dst, const void *src, size_t bytes);  /* async */
int lslam_d2d(lslam_ctx *ctx, void *dst, const void *src, size_t bytes);  /* async */
int lslam_memset(lslam_ctx *ctx, void *dst, int value, size_t bytes);     /* async */
/* Page-lock existing host memory (hipHostRegister), e.g. a host batch shared between the
 * ranks of one node (the reference's mp.Queue hand-off, SLAM.py:13,18-23, done as shared
 * memory + per-rank H2D of a shard): lslam_h2d / lslam_d2h from it then run at PCIe rate. */
int lslam_host_register(void *hptr, size_t bytes);
int lslam_host_unregister(void *hptr);
/* The context's main HIP stream (a hipStream_t).  Work a caller enqueues on it, e.g. an RCCL
 * gather of a pipeline call's outputs (lidar_slam_amd/collective.py), runs after every call made
 * on the context so far and before later ones.  It must not write a buffer a later call's MT
 * producer reads (seeds, CSR offsets, mt_state_in) unless followed by lslam_sync. */
int lslam_ctx_stream(lslam_ctx *ctx, void **stream);
/* sizes (bytes) of the ABI structs as compiled into the library, in this order:
 * lslam_chunk_model, lslam_landmark, lslam_ransac_params, lslam_ukf_params, lslam_scan_batch,
 * lslam_express_measures, lslam_express_revs, lslam_match_params, lslam_match_batch.  Writes
 * min(n, 9) entries, returns 9. */
int lslam_abi_sizes(int64_t *sizes, int n);
/* the same for the structs added since: lslam_grid_params, lslam_grid_batch.  Writes min(n, 2)
 * entries, returns 2. */
int lslam_grid_abi_sizes(int64_t *sizes, int n);
/* and for lslam_mapmatch_params, lslam_mapmatch_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_mapmatch_abi_sizes(int64_t *sizes, int n);
/* and for lslam_mapfuse_params, lslam_mapfuse_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_mapfuse_abi_sizes(int64_t *sizes, int n);
/* and for lslam_reloc_params, lslam_reloc_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_reloc_abi_sizes(int64_t *sizes, int n);
/* and for lslam_raycast_params, lslam_raycast_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_raycast_abi_sizes(int64_t *sizes, int n);
/* and for lslam_recentre_params, lslam_recentre_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_recentre_abi_sizes(int64_t *sizes, int n);
/* and for lslam_dist_params, lslam_dist_batch, lslam_fieldscore_params, lslam_fieldscore_batch.
 * Writes min(n, 4) entries, returns 4. */
int lslam_dist_abi_sizes(int64_t *sizes, int n);
/* and for lslam_fieldalign_params, lslam_fieldalign_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_fieldalign_abi_sizes(int64_t *sizes, int n);
/* and for lslam_fieldfuse_params, lslam_fieldfuse_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_fieldfuse_abi_sizes(int64_t *sizes, int n);
/* and for lslam_relocprior_params, lslam_relocprior_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_relocprior_abi_sizes(int64_t *sizes, int n);
/* and for lslam_page_params, lslam_page_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_page_abi_sizes(int64_t *sizes, int n);
/* per-kernel HIP-event timing on the ctx stream (kernel ids: LSLAM_K_*) */
enum { LSLAM_K_POLAR = 0, LSLAM_K_HYP = 1, LSLAM_K_PIPELINE = 2, LSLAM_K_LANDMARK = 3, LSLAM_K_UKF = 4,
       LSLAM_K_RNG = 5 /* parity-stream producer */, LSLAM_K_CONSENSUS = 6 /* per-chunk A4-A8 */,
       LSLAM_K_EXPRESS = 7 /* a whole express decode / scans call */,
       LSLAM_K_EXPRESS_SCATTER = 8 /* its decode + A1 + scatter kernel */,
       LSLAM_K_MATCH = 9 /* a whole scan-match call */, LSLAM_K_GRID = 10 /* a whole grid update */,
       LSLAM_K_MAPMATCH = 11 /* a whole scan-to-map call */, LSLAM_K_MAPFUSE = 12 /* a whole match-fusion call */,
       LSLAM_K_RELOC = 13 /* a whole relocalisation call */, LSLAM_K_RAYCAST = 14 /* a whole grid ray-cast call */,
       LSLAM_K_RECENTRE = 15 /* a whole grid recentre call */, LSLAM_K_COUNT = 16 };
int lslam_set_timing(lslam_ctx *ctx, int enable);
/* which kernel ids are timed while timing is on (bit k = LSLAM_K_k; default all).  Timing
 * events between the producer and consumer kernels change how the two streams overlap,
 * so a throughput measurement should time only the kernel it reports. */
int lslam_set_timing_mask(lslam_ctx *ctx, uint32_t mask);
int lslam_timing(lslam_ctx *ctx, int kernel, double *total_ms, int64_t *launches);  /* syncs */
int lslam_timing_reset(lslam_ctx *ctx);
/* Bytes of Fisher-Yates steps scratch per producer slot (two slots; default 2 GiB, or the
 * LSLAM_STEPS_BUDGET environment variable).  A parity-mode call whose scans are one chunk each
 * (C5) and whose steps exceed it runs the producer in epochs of as many draws as fit, each
 * resolved before its slot is reused.  bytes <= 0 restores the default.  Syncs. */
int lslam_set_steps_budget(lslam_ctx *ctx, int64_t bytes);
/* Bytes of coarse-score scratch of a relocalisation call (default: the score volume of a 4096-robot
 * map match at its defaults, 296 MB, or the LSLAM_RELOC_BUDGET environment variable).  A call whose
 * coarse volumes exceed it runs its coarse stage in chunks of as many robots as fit (at least one);
 * the results do not depend on it.  bytes <= 0 restores the default. */
int lslam_set_reloc_budget(lslam_ctx *ctx, int64_t bytes);

/* ---- host helpers ---- */
int lslam_ransac_params_default(lslam_ransac_params *p);
int lslam_ukf_params_default(lslam_ukf_params *p, int32_t n_landmarks);
int lslam_match_params_default(lslam_match_params *p);
int lslam_grid_params_default(lslam_grid_params *p);
int lslam_mapmatch_params_default(lslam_mapmatch_params *p);
int lslam_mapfuse_params_default(lslam_mapfuse_params *p);
int lslam_reloc_params_default(lslam_reloc_params *p);
int lslam_raycast_params_default(lslam_raycast_params *p);
int lslam_recentre_params_default(lslam_recentre_params *p);
int lslam_dist_params_default(lslam_dist_params *p);
int lslam_fieldscore_params_default(lslam_fieldscore_params *p);
int lslam_fieldalign_params_default(lslam_fieldalign_params *p);
int lslam_fieldfuse_params_default(lslam_fieldfuse_params *p);
int lslam_relocprior_params_default(lslam_relocprior_params *p);
int lslam_page_params_default(lslam_page_params *p);
/* smallest e with RN(sqrt(e)) >= thr: (residual < thr) <=> (squared residual < cutoff) */
double lslam_inlier_cutoff(double thr);
/* MerweScaledSigmaPoints weights (filterpy _compute_weights) for n = 3 */
int lslam_ukf_weights(const lslam_ukf_params *p, double *Wm7, double *Wc7, double *lambda_plus_n);
/* numpy RandomState(seed) state: key[624] + pos (host memory, 625 words) */
int lslam_mt_seed_state(uint32_t seed, uint32_t *state625);

/* ---- hot path (device pointers, async on the ctx stream) ---- */
/* A1: xy[i] = (d cos(-th*pi/180 + pi/2), d sin(...)); n measures */
int lslam_polar_to_xy(lslam_ctx *ctx, const double *theta_deg, const double *dist, double *xy, int64_t n);
/* E1: RPLidar express packets (M x 84 bytes, 4-byte aligned) -> measure stream */
int lslam_express_decode(lslam_ctx *ctx, const uint8_t *packets, int64_t n_packets, const lslam_express_measures *out);
/* E1 + A1 + A2: packets -> revolutions of chunked xy (functions.py:56-76); the first
 * `skip` measures of packet 0 are dropped (a resumed stream).  Writes are clipped
 * to the capacities; counts always holds the required sizes. */
int lslam_express_scans(lslam_ctx *ctx, const uint8_t *packets, int64_t n_packets, int32_t skip,
                        const lslam_express_revs *out);
/* A3: the draws each chunk's ransac would make, assuming no early stop
 * (draws_out [n_chunks][max_trials+1][2]).  Uses b->seeds/mt_state_in/mt_state_out. */
int lslam_hyp_mt19937(lslam_ctx *ctx, const lslam_scan_batch *b, int32_t max_trials);
/* A3-A8: ransac per chunk (chained RNG per scan), masks, models */
int lslam_ransac(lslam_ctx *ctx, const lslam_scan_batch *b, const lslam_ransac_params *p);
/* A9-A10: association over b->models (already fitted) + y_proj */
int lslam_landmarks(lslam_ctx *ctx, const lslam_scan_batch *b, const lslam_ransac_params *p);
/* U1-U8: one predict and/or update per scan */
int lslam_ukf_step(lslam_ctx *ctx, const lslam_scan_batch *b, const lslam_ukf_params *u);
/* Test / diagnostic: lslam_ukf_step (the same kernel code, lane-group form) that also writes the
 * update's intermediate values per scan to trace (device, [n_scans][42 + 32 L] doubles, m = 2L):
 *   [0, 21)            sigma points sigma_k (k = 0..6, [x, y, theta])
 *   [21, 42)           residual_x(sigma_k, x)                           UKFMethods.py:60-63
 *   [42, 42 + 7m)      hx(sigma_k) = transfer_function(sigma_k, lmk)    UKFMethods.py:26-34
 *   [42 + 7m, +m)      zp (z_mean about sigma 0)
 *   [42 + 8m, +m)      residual_h(z, zp)                                UKFMethods.py:66-71
 *   [42 + 9m, +7m)     residual_h(hx(sigma_k), zp)
 * Entries of inactive landmark slots are not written.  Needs LSLAM_UKF_UPDATE; not in MAP mode. */
int lslam_ukf_trace(lslam_ctx *ctx, const lslam_scan_batch *b, const lslam_ukf_params *u, double *trace);
/* A3-A10 (+ U1-U8 if u != NULL) for every scan of the batch in one call: MT19937 producer (its
 * own stream, overlapping the previous call's consumers), resolve, consensus, fix-up, then the
 * association / UKF post pass */
int lslam_scan_pipeline(lslam_ctx *ctx, const lslam_scan_batch *b, const lslam_ransac_params *p,
                        const lslam_ukf_params *u);
/* LiDAR-only odometry: a correlative scan match per robot, previous revolution (ref) against the
 * current one (cur), giving the pose of the current frame in the previous one, q ~ R(theta) p + t.
 * FP64, every operation rounded on its own; half = grid_w/2, inv = 1.0/cell, Nt = 2 k_trans + 1,
 * Ntheta = 2 k_theta + 1.  A point is valid if both coordinates are finite and it is not exactly
 * (0, 0) (the express decoder's invalid measure).
 *   1. grid G [grid_w][grid_w]: a valid ref point with fx = floor(x inv), fy = floor(y inv), both
 *      in [-half, half) (compared as doubles), occupies cell (fy + half, fx + half);
 *      G[c] = max(0, smear + 1 - Chebyshev distance from c to the nearest occupied cell).
 *   2. scores S[k][jy][jx] (int32): with (c, s) = rot[k], for each valid cur point
 *      x' = c x - s y, y' = s x + c y, ax = floor(x' inv), ay = floor(y' inv);
 *      S = sum of G[ay + (jy - k_trans) + half][ax + (jx - k_trans) + half], 0 outside the grid.
 *   3. winner: the highest score, then the smallest d2 = (k - k_theta)^2 + (jy - k_trans)^2 +
 *      (jx - k_trans)^2, then the smallest flat index (k Nt + jy) Nt + jx.
 *   4. per axis, with the winner's neighbours s-, s+ and its score s0: den = s- - 2 s0 + s+; off
 *      the window's border and with den < 0 the offset is 0.5 (s- - s+) / den, else 0.
 *   5. delta = ((jx - k_trans + ox) cell, (jy - k_trans + oy) cell, (k - k_theta + ot) theta_step),
 *      best = (k, jy, jx, score); LSLAM_MATCH_EDGE if the winner is on the border along some axis;
 *      a winning score of 0 gives LSLAM_MATCH_EMPTY alone, delta = 0, best = the centre.
 *   6. with u != NULL and ukf_u given, the wheel speeds that UKFMethods.py:17-24 (x += dt B(theta) u)
 *      turns back into (tx, dtheta): a = tx / (wheel_radius dt), b = dtheta wheel_base /
 *      (2 wheel_radius dt), ukf_u = (a - b, a + b); (0, 0) when EMPTY.  ty stays in delta only.
 * Runs on the context's main stream, after every earlier call.  Out-of-range parameters and
 * missing required pointers return LSLAM_ERR_ARG; n_scans == 0 does nothing. */
int lslam_scan_match(lslam_ctx *ctx, const lslam_match_batch *b, const lslam_match_params *p,
                     const lslam_ukf_params *u);
/* Occupancy-grid mapping: one revolution per robot and the robot's pose -> the robot's grid of
 * clamped log-odds (the inverse sensor model: the cells a beam crosses are free, the cell it ends
 * in is occupied).  Per robot r, in FP64 with every operation rounded on its own, inv = 1.0 / cell:
 *   0. pose and rotation: (px, py, theta) = pose[r], (ox, oy) = origin[r], the world coordinates of
 *      the corner of cell (0, 0).  The library computes (c, s) = (cos theta, sin theta) and writes
 *      them to rot[r] (always, NaN for a non-finite theta); the written bits are the definition's
 *      input from here on.  Robot cell, as doubles: X0 = floor((px - ox) inv),
 *      Y0 = floor((py - oy) inv).  If any of the five inputs is not finite, or |X0| or |Y0| >= 2^20:
 *      flags[r] = LSLAM_GRID_BAD_POSE, n_used[r] = (0, 0) and the robot's grid is not touched.
 *   1. points: valid as in lslam_scan_match (both coordinates finite, not exactly (0, 0)).  A valid
 *      point with x x + y y > max_range max_range is counted in n_used[r][1] and ignored.  The
 *      others are counted in n_used[r][0]; for them wx = px + (c x - s y), wy = py + (s x + c y),
 *      X1 = floor((wx - ox) inv), Y1 = floor((wy - oy) inv).
 *   2. ray, in integers: dx = X1 - X0, dy = Y1 - Y0, n = max(|dx|, |dy|).  The free cells are
 *      i = 0 .. n-1: (X0 + sgn(dx) ((2 i |dx| + n) div 2n), Y0 + sgn(dy) ((2 i |dy| + n) div 2n));
 *      the hit cell is (X1, Y1); with n = 0 there is only the hit.  The form is closed on purpose:
 *      every cell of a ray is independent of the others, so lanes can share a ray and a tile can
 *      clip a ray to an i-interval.  max_range / cell <= 4096 keeps 2 i |d| + n far inside int32.
 *   3. per-revolution sum: D[Y][X] = l_hit (rays that hit the cell) + l_miss (rays that pass it
 *      free), over the cells inside [0, grid_w)^2; cells outside are ignored.  LSLAM_GRID_CLIPPED is
 *      set iff some cell of some ray lies outside: n_used[r][0] > 0 and the robot cell is outside,
 *      or some hit cell is outside (a ray's cells lie in the bounding box of its two ends).
 *   4. update, once per call: where D != 0, L' = clamp(L + D, l_min, l_max); every other cell keeps
 *      its value, including a value outside the clamp range that the caller put there.  L is
 *      int16 [n_robots][grid_w][grid_w], row Y, in units of 0.01 nat.  The sum is taken before the
 *      single clamp, so the result does not depend on the order of rays or atomics.
 * Runs on the context's main stream, after every earlier call: it sees the ukf_x that a preceding
 * lslam_scan_pipeline or lslam_ukf_step wrote, and reads xy in place.  Out-of-range parameters and
 * missing pointers return LSLAM_ERR_ARG (the message names the field), checked before the context
 * is touched; n_robots == 0 does nothing. */
int lslam_grid_update(lslam_ctx *ctx, const lslam_grid_batch *b, const lslam_grid_params *p);
/* Scan-to-map matching: one revolution per robot, a pose guess and the robot's log-odds grid -> the
 * pose that best lays the revolution onto the occupied cells: the correlative search of
 * lslam_scan_match with the map in the place of the previous revolution, in the world frame.  The
 * grid's geometry is g's cell and grid_w (g is checked as lslam_grid_update checks it).  Per robot r,
 * in FP64 with every operation rounded on its own, then integers; inv = 1.0 / cell, half = win_w/2,
 * Nt = 2 k_trans + 1, Ntheta = 2 k_theta + 1:
 *   0. robot cell: (px, py, theta) = pose[r], (ox, oy) = origin[r].  The library computes
 *      (c, s) = (cos theta, sin theta) and writes them to rot0[r] (always, NaN for a non-finite
 *      theta); the written bits are the definition's input.  X0 = floor((px - ox) inv),
 *      Y0 = floor((py - oy) inv).  The pose is bad under the condition of lslam_grid_update step 0;
 *      then flags[r] = LSLAM_MAPMATCH_BAD_POSE, delta = 0, best = (k_theta, k_trans, k_trans, 0),
 *      n_valid = (0, 0), pose_out = pose bit for bit, and scores (if given) are zeros.
 *   1. look-up grid G [win_w][win_w]: window cell (gy, gx) is map cell (Y0 - half + gy,
 *      X0 - half + gx); it is occupied iff that cell lies in [0, grid_w)^2 and L >= occ_min.
 *      G[c] = max(0, smear + 1 - Chebyshev distance from c to the nearest occupied window cell):
 *      the smear is clipped to the window, as in lslam_scan_match step 1.  n_valid[r][0] = the number
 *      of occupied window cells.
 *   2. scores S[k][jy][jx] (int32): with (ck, sk) = rot[k], cc = c ck - s sk, ss = s ck + c sk.
 *      Points are valid as in lslam_scan_match; there is no max_range cut.  For a valid point
 *      wx = px + (cc x - ss y), wy = py + (ss x + cc y), X1 = floor((wx - ox) inv),
 *      Y1 = floor((wy - oy) inv), ax = X1 - X0, ay = Y1 - Y0; the point counts iff both lie in
 *      [-half - k_trans, half + k_trans) (compared as doubles).  S = the sum over those points of
 *      G[ay + (jy - k_trans) + half][ax + (jx - k_trans) + half], 0 outside the window.
 *      n_valid[r][1] = the number of valid points.
 *   3. winner, parabola per axis, best, EMPTY and EDGE: steps 3-5 of lslam_scan_match.
 *      delta = ((jx - k_trans + ox') cell, (jy - k_trans + oy') cell, (k - k_theta + ot') theta_step),
 *      with the parabola offsets ox', oy', ot', is a world-frame correction of the guess.
 *   4. gate, in int64: LSLAM_MAPMATCH_WEAK iff not EMPTY and
 *      1000 score < min_permille (smear + 1) n_valid[r][1].
 *   5. pose_out[r] = (px + delta[0], py + delta[1], theta + delta[2]), one addition each, no angle
 *      wrap, iff none of EMPTY, BAD_POSE, WEAK is set; otherwise pose_out[r] = pose[r] bit for bit.
 *      EDGE alone still applies the correction; delta and best are reported in every case.
 *      pose_out may be pose itself: the thread that writes a robot's pose_out has read its pose.
 * Runs on the context's main stream, after every earlier call: it sees the ukf_x of a preceding
 * lslam_scan_pipeline and the grid of a preceding lslam_grid_update.  Out-of-range parameters and
 * missing pointers return LSLAM_ERR_ARG (the message names the field), checked before the context
 * is touched; n_robots == 0 does nothing. */
int lslam_map_match(lslam_ctx *ctx, const lslam_mapmatch_batch *b, const lslam_grid_params *g,
                    const lslam_mapmatch_params *m);
/* Match fusion: lslam_map_match as a measurement update of the filter.  The match is turned into a
 * measurement z of the pose with a covariance Rm taken from the whole score volume, and (x, P) =
 * (m.pose, P) is updated by a Kalman step, gated on the innovation's Mahalanobis distance under the
 * filter's own uncertainty.  Per robot r:
 *   0-4. steps 0-4 of lslam_map_match, verbatim, with b->m, g and m: robot cell, G, score volume S,
 *      winner (k*, jy*, jx*, s0), parabola, delta, best, n_valid, rot0, EMPTY, EDGE, BAD_POSE, WEAK.
 *      With EMPTY or BAD_POSE set, steps 5-7 are skipped and no further flag is set: moments, Rm and
 *      nis are zeros, z = pose bit for bit.
 *   5. moments, all int64: cut = (s0 cut_permille) div 1000.  Every candidate (k, jy, jx) of the
 *      volume weighs w = max(0, S - cut) at the offsets a = jx - jx*, b = jy - jy*, c = k - k*;
 *      moments[r] = (W = sum w, sum wa, sum wb, sum wc, sum waa, sum wab, sum wac, sum wbb, sum wbc,
 *      sum wcc).  Integer sums do not depend on the order.  cut < s0, so W >= 1.  With scores below
 *      2^31, |a|, |b| <= 30, |c| <= 62 and at most 63 * 31 * 31 candidates, every sum stays below
 *      5e17 in magnitude, inside int64 and converted to double with one rounding.
 *   6. match covariance, FP64, every operation rounded on its own.  Wd = (double)W; with the axes
 *      (0, 1, 2) = (a, b, c): mean_i = (double)(sum w i) / Wd, and for i <= j
 *      C_ij = (double)(sum w i j) / Wd - mean_i mean_j.  With sc = (cell, cell, theta_step):
 *      Rm_ij = (C_ij sc_i) sc_j; on the diagonal Rm_ii = (C_ii sc_i) sc_i + (sc_i sc_i) / 12.0, the
 *      variance of one search quantum, so that Rm is never singular; then Rm_ij = Rm_ij r_scale, and
 *      Rm_ji = Rm_ij.  z = (px + delta[0], py + delta[1], theta + delta[2]), no angle wrap.
 *   7. innovation and gate.  y = delta (the guess is the mean).  S_ij = P_ij + Rm_ij, all nine.  The
 *      adjugate A of S, every entry of the form p q - r s (two products, one subtraction):
 *        A00 = S11 S22 - S12 S21   A01 = S02 S21 - S01 S22   A02 = S01 S12 - S02 S11
 *        A10 = S12 S20 - S10 S22   A11 = S00 S22 - S02 S20   A12 = S02 S10 - S00 S12
 *        A20 = S10 S21 - S11 S20   A21 = S01 S20 - S00 S21   A22 = S00 S11 - S01 S10
 *      det = (S00 A00 + S01 A10) + S02 A20.  LSLAM_MAPFUSE_BAD_COV iff some entry of P is not finite,
 *      or not (S00 > 0 and A22 > 0 and det > 0 and det finite); then nis = 0.0 and the rest of this
 *      step is skipped.  Otherwise Si_ij = A_ij / det, v_i = (Si_i0 y0 + Si_i1 y1) + Si_i2 y2,
 *      nis = (y0 v0 + y1 v1) + y2 v2, and LSLAM_MAPFUSE_OUTLIER iff not (nis <= nis_max).
 *   8. update, iff none of EMPTY, BAD_POSE, WEAK, BAD_COV, OUTLIER is set (EDGE alone still updates).
 *      Every element of a 3x3 product is (t0 + t1) + t2.  K = P Si, K_ij = (P_i0 Si_0j + P_i1 Si_1j)
 *      + P_i2 Si_2j.  pose_out_i = x_i + ((K_i0 y0 + K_i1 y1) + K_i2 y2).  Joseph form:
 *      A = I - K (A_ij = 1.0 - K_ij on the diagonal, 0.0 - K_ij off it), AP = A P,
 *      U_ij = (AP_i0 A_j0 + AP_i1 A_j1) + AP_i2 A_j2, KR = K Rm, V_ij = (KR_i0 K_j0 + KR_i1 K_j1)
 *      + KR_i2 K_j2, T = U + V, P_out_ij = 0.5 (T_ij + T_ji).
 *      In every other case pose_out and P_out are pose and P bit for bit (copied as 64-bit words: a
 *      NaN keeps its payload).  delta, best, n_valid, rot0, flags, and for WEAK, OUTLIER and BAD_COV
 *      also z, Rm, nis and moments are reported as computed.
 * pose_out may be pose and P_out may be P: the one thread that writes a robot's outputs has read its
 * pose and P first.  Runs on the context's main stream as lslam_map_match does.  Out-of-range
 * parameters and missing pointers return LSLAM_ERR_ARG (the message names the field), checked before
 * the context is touched; n_robots == 0 does nothing. */
int lslam_map_fuse(lslam_ctx *ctx, const lslam_mapfuse_batch *b, const lslam_grid_params *g,
                   const lslam_mapmatch_params *m, const lslam_mapfuse_params *f);

/* Global relocalisation: one revolution per robot and the robot's log-odds grid, NO pose guess -> the
 * pose in the whole grid, over all headings, that best lays the revolution onto the map; LOST if there
 * is none, AMBIGUOUS if there are two.  A coarse correlative search over every coarse cell and every
 * heading, the K best separated peaks refined by lslam_map_match, then a selection.  g and m are
 * checked as lslam_map_match checks them, q as its table says; the fine window must cover one coarse
 * quantum: 2 m.k_trans >= q.factor and 2 m.k_theta m.theta_step >= q.head_step.  Per robot r, in FP64
 * with every operation rounded on its own, then integers; f = q.factor, Wc = grid_w / f,
 * cellc = cell f, invc = 1.0 / cellc, K = q.n_cand:
 *   0. coarse map: C[cy][cx] = 1 iff some fine cell of the f x f block (rows f cy .. f cy + f - 1,
 *      likewise columns) holds L >= m.occ_min.  n_occ[r] = the number of set coarse cells.
 *   1. points: valid as in lslam_scan_match (both coordinates finite, not exactly (0, 0)); only valid
 *      points with x x + y y <= max_range max_range are used (lslam_grid_update step 1).
 *      n_used[r] = their count.
 *   2. coarse scores Sc[k][ty][tx] (int32), k in [0, n_head), ty, tx in [0, Wc): with
 *      (c, s) = head_rot[k], the caller's bits for the heading (double)k head_step, for each used
 *      point x' = c x - s y, y' = s x + c y, ax = floor(x' invc + 0.5), ay = floor(y' invc + 0.5);
 *      the point counts iff -Wc < ax < Wc and -Wc < ay < Wc (compared as doubles).  Sc = the sum over
 *      those points of C[ty + ay][tx + ax], 0 outside the coarse grid: the robot at the centre of
 *      coarse cell (ty, tx).
 *   3. peaks: candidates are ordered by score, highest first, then by the smaller flat index
 *      (k Wc + ty) Wc + tx.  A candidate is a peak iff its score is > 0 and it comes before all of its
 *      up to 26 neighbours in that order; heading neighbours are k +- 1 mod n_head, translation
 *      neighbours outside the coarse grid do not exist.  The first K peaks in that order are the
 *      candidates j = 0 .. K-1: cand[j][r] = (k, ty, tx, score), cand_pose[j][r] =
 *      (ox + ((double)tx + 0.5) cellc, oy + ((double)ty + 0.5) cellc, (double)k head_step).  Missing
 *      ranks get cand = (-1, -1, -1, 0) and a pose of three quiet NaNs.  The layout is [K][n_robots],
 *      so rank j is a plain [n_robots][3] pose array.
 *   4. fine stage: for each rank j, lslam_map_match steps 0-5 exactly as written, with
 *      pose = cand_pose[j], the robot's grid and origin, and m; its outputs go to fine_pose[j],
 *      fine_delta[j], fine_best[j], fine_nvalid[j], fine_rot0[j], fine_flags[j].  A NaN pose gives
 *      BAD_POSE by that definition's rule.
 *   5. selection: rank j is eligible iff fine_flags[j] & (EMPTY | BAD_POSE | WEAK) == 0.  The winner
 *      is the eligible rank with the highest fine_best[j][3], then the lowest j.  With no eligible
 *      rank flags[r] = LSLAM_RELOC_LOST.  A rival is an eligible rank other than the winner that is
 *      not a duplicate of it: with the refined poses a and b, dt = fabs(a.theta - b.theta), and
 *      dt = two_pi - dt if dt > pi (the double literals 3.141592653589793 and 6.283185307179586); the
 *      rank is a duplicate iff fabs(a.x - b.x) <= dup_mm, fabs(a.y - b.y) <= dup_mm and dt <= dup_rad.
 *      The best rival is the one with the highest fine score, then the lowest j.
 *      LSLAM_RELOC_AMBIGUOUS iff some rival has 1000 score_rival >= ambig_permille score_winner (int64).
 *      result[r] = (winner rank, its k, ty, tx, its coarse score, its fine score, the best rival's
 *      rank or -1, that rival's fine score or 0); with LOST (-1, -1, -1, -1, 0, 0, -1, 0).
 *   6. outputs: iff neither LOST nor AMBIGUOUS, pose_out[r] = the winner's fine_pose, three doubles
 *      copied bit for bit, and (if P_out is given) P_out[r] = diag(sxy sxy, sxy sxy, sth sth) from
 *      reset_sigma_xy and reset_sigma_theta, the products taken once on the host, zeros off the
 *      diagonal.  Otherwise pose_out[r] and P_out[r] keep their bits.  pose_out may be the filter's
 *      ukf_x and P_out its ukf_P.
 * coarse_scores, if given, receives Sc.  The coarse volume is otherwise held in a scratch of bounded
 * size and the robots go through the coarse stage in chunks (lslam_set_reloc_budget); no result
 * depends on that.  Runs on the context's main stream as lslam_map_match does.  Out-of-range
 * parameters and missing pointers return LSLAM_ERR_ARG (the message names the field), checked before
 * the context is touched; n_robots == 0 does nothing. */
int lslam_map_relocalize(lslam_ctx *ctx, const lslam_reloc_batch *b, const lslam_grid_params *g,
                         const lslam_mapmatch_params *m, const lslam_reloc_params *q);

/* Grid ray casting: one revolution per robot, the robot's pose and its log-odds grid -> for every beam
 * where the MAP says it stops, and how that compares with where it returned.  The read side of
 * lslam_grid_update: the same pose, points and integer ray, walked until the map ends it.  The grid's
 * geometry is g's cell, grid_w and max_range (g is checked as lslam_grid_update checks it).  A cell is
 * occupied iff L >= occ_min, free iff L <= free_max; every other cell, and every cell off the map, is
 * unknown.  Per robot r, in FP64 with every operation rounded on its own, then integers;
 * inv = 1.0 / cell:
 *   0. pose, rotation and robot cell: step 0 of lslam_grid_update, verbatim; (c, s) go to rot[r]
 *      (always) and the written bits are the definition's input.  X0d = floor((px - ox) inv),
 *      Y0d = floor((py - oy) inv) as doubles, (X0, Y0) as integers.  A bad pose (that step's condition)
 *      gives flags[r] = LSLAM_RAYCAST_BAD_POSE, cls = 0 and stop = (0, 0, 0) for every point of the
 *      robot, and counts[r] all zero.  Otherwise flags[r] = 0.
 *   1. points: valid as in lslam_scan_match (both coordinates finite, not exactly (0, 0)); an invalid
 *      point has cls = LSLAM_RAYCAST_INVALID and stop = (0, 0, 0).  A valid point is beyond iff
 *      x x + y y > max_range max_range.  A valid point that is not beyond has the measured hit cell
 *      (X1, Y1) of lslam_grid_update step 1, and its measured step i_m = max(|X1 - X0|, |Y1 - Y0|).
 *   2. far cell of the beam: m = max(|x|, |y|), far = max_range + 2.0 cell, q = far / m, fx = x q,
 *      fy = y q: the beam scaled to the square of half side far, its exact direction for one division.
 *      wx = px + (c fx - s fy), wy = py + (s fx + c fy), XFd = floor((wx - ox) inv),
 *      YFd = floor((wy - oy) inv), Dxd = XFd - X0d, Dyd = YFd - Y0d, all doubles.  If Dxd or Dyd is
 *      not finite or exceeds 8192 in magnitude (a denormal point: q overflows) the point is INVALID as
 *      in step 1.  Otherwise Dx = (int)Dxd, Dy = (int)Dyd, n = max(|Dx|, |Dy|).
 *   3. walk i = 0 .. n.  The offset at step i is (ox, oy) = (sgn(Dx) ((2 i |Dx| + n) div 2n),
 *      sgn(Dy) ((2 i |Dy| + n) div 2n)), the ray of lslam_grid_update step 2; n = 0 means i = 0 only,
 *      offset (0, 0).  Rc = (int)floor(max_range inv).  The walk stops at the first step that meets
 *      one of these, tested in this order:
 *        ox ox + oy oy > Rc Rc                      kind NONE: the ray left the range circle still free
 *        the cell (X0 + ox, Y0 + oy) is occupied    kind OCC
 *        it is unknown, or off the map              kind UNKNOWN
 *      and i_h is that step.  If no step stops it: kind NONE, i_h = n + 1, (ox, oy) of step n.
 *      stop[p] = (ox, oy, i_h).  (|ox|, |oy| <= 8192 keeps every product inside int32.)
 *   4. class, in integers; i_m counts as +infinity for a beyond point:
 *        OCC      i_m < i_h - tol: NOVEL;  i_m > i_h + tol: THROUGH;  otherwise MATCH
 *        UNKNOWN  i_m < i_h - tol: NOVEL;  otherwise UNMAPPED
 *        NONE     beyond, or i_m >= i_h - tol: MATCH;  otherwise NOVEL
 *      cls[p] = class | kind << 4.
 *   5. counts[r] = (points of class 0, 1, 2, 3, 4, points that are beyond and not INVALID, points of
 *      kind NONE that are not INVALID, 0): integers, so the order of accumulation does not matter.
 * The expected range of a beam of kind OCC is cell hypot(ox, oy).  To render the map as a scan, pass
 * unit vectors times max_range: stop is the answer and the classes are ignored.
 * Runs on the context's main stream, after every earlier call: it sees the ukf_x of a preceding
 * lslam_scan_pipeline and the grid of a preceding lslam_grid_update.  Out-of-range parameters and
 * missing pointers return LSLAM_ERR_ARG (the message names the field), checked before the context is
 * touched; n_robots == 0 does nothing. */
int lslam_grid_raycast(lslam_ctx *ctx, const lslam_raycast_batch *b, const lslam_grid_params *g,
                       const lslam_raycast_params *p);

/* Grid recentre: the rolling map.  Each robot's grid and its origin are shifted by whole cells, in
 * place, so that the robot's cell comes back to the middle; what scrolls off is lost (there is no
 * archive of the strip that leaves) and what scrolls in is unknown.  Every reader of the grid takes
 * origin as a device pointer and follows.  The grid's geometry is g's cell and grid_w (g is checked as
 * lslam_grid_update checks it), W = grid_w, inv = 1.0 / cell; margin <= W / 2.  Per robot r, in FP64
 * with every operation rounded on its own, then integers:
 *   0. robot cell and bad poses: X0d = floor((px - ox) inv), Y0d = floor((py - oy) inv), and the
 *      condition of a bad pose, are step 0 of lslam_grid_update (a non-finite pose component or
 *      origin, or |X0d| or |Y0d| >= 2^20).  A bad pose leaves grid and origin untouched:
 *      shift[r] = (0, 0), flags[r] = LSLAM_RECENTRE_BAD_POSE.  Otherwise (X0, Y0) are the integers.
 *   1. the shift.  If margin <= X0 < W - margin and margin <= Y0 < W - margin: (sx, sy) = (0, 0).
 *      Otherwise both axes are recentred: s = quantum floordiv(c - W div 2 + quantum div 2, quantum)
 *      for c = X0, Y0, where floordiv rounds toward minus infinity and the halves are integer halves.
 *   2. a shift of (0, 0), also one that step 1 triggered and rounded to zero, writes shift[r] = (0, 0)
 *      and flags[r] = 0 and nothing else: logodds and origin keep every bit.
 *   3. the new origin, per axis: origin' = fl(origin + fl(s cell)), two roundings, no fused
 *      multiply-add.  If origin' is not finite the robot is a bad pose as in step 0.
 *   4. the new grid: L'[y][x] = L[y + sy][x + sx] where that source cell is on the map, 0 (unknown)
 *      elsewhere.  Cells move as 16-bit patterns: nothing is clamped, values outside [l_min, l_max]
 *      survive.  flags[r] = LSLAM_RECENTRE_MOVED, and | LSLAM_RECENTRE_CLEARED when |sx| >= W or
 *      |sy| >= W (nothing is kept).
 *   5. shift[r] = (sx, sy); origin[r] = origin'; logodds in place.
 * The world square of a cell that stays on the map is the same before and after, up to the two
 * roundings of step 3 (none when origin is a multiple of cell that FP64 holds exactly).
 * Runs on the context's main stream, after every earlier call and before every later one: it sees the
 * ukf_x of a preceding lslam_scan_pipeline, and a following lslam_grid_update, lslam_map_match,
 * lslam_map_fuse, lslam_map_relocalize or lslam_grid_raycast sees the moved grid and origin.
 * Out-of-range parameters and missing pointers return LSLAM_ERR_ARG (the message names the field),
 * checked before the context is touched; n_robots == 0 does nothing. */
int lslam_grid_recentre(lslam_ctx *ctx, const lslam_recentre_batch *b, const lslam_grid_params *g,
                        const lslam_recentre_params *p);

/* The paged rolling grid: a world canvas behind each robot's window.  lslam_grid_recentre loses what
 * scrolls off; with a canvas the strip that leaves is written there and the strip that enters is read
 * from there, so a robot that comes back finds its room.  New per-robot state, in device memory:
 *   canvas[n_robots][Cw][Cw] int16, row Y, Cw = canvas_w (pp, 16..2048);
 *   win[n_robots][2] int32 in/out, (wx, wy): the canvas coordinates of window cell (0, 0).  It may be
 *   negative or beyond the canvas: the window may hang off the canvas partly or wholly.
 * Window cell (x, y) is ON THE CANVAS iff 0 <= wx + x < Cw and 0 <= wy + y < Cw, tested in 64-bit
 * arithmetic (win itself is 32 bits; win + shift is stored as its low 32 bits).
 *
 * lslam_grid_recentre_paged: recentre batch b, page batch pg (the same n_robots), g, p as
 * lslam_grid_recentre takes them, and pp.  W = grid_w, L = logodds.  Per robot r:
 *   1. steps 0 to 3 of lslam_grid_recentre exactly as written there: robot cell, bad pose, shift
 *      (sx, sy), new origin with its non-finite case.  A bad pose or a shift of (0, 0) changes nothing
 *      in logodds, origin, canvas or win; moved[r] = (0, 0) and pg.flags[r] = 0, and b's shift[r] and
 *      flags[r] are what lslam_grid_recentre writes.
 *   2. store.  Every window cell (x, y) whose destination (x - sx, y - sy) is off the window leaves
 *      it.  On the canvas: canvas[wy + y][wx + x] = L[y][x], the 16-bit pattern.  Off the canvas: it
 *      is dropped, and pg.flags[r] |= LSLAM_PAGE_LOST.
 *   3. shift.  L'[y][x] = L[y + sy][x + sx] where that source is on the window (step 4 of
 *      lslam_grid_recentre).  Every other cell (x, y) ENTERS: it takes
 *      canvas[wy + sy + y][wx + sx + x] if that cell is on the canvas, 0 otherwise.
 *   4. win[r] = win[r] + (sx, sy); moved[r] = (cells stored in step 2, cells loaded from the canvas in
 *      step 3); b's shift[r], flags[r] (MOVED, CLEARED) and origin[r] as lslam_grid_recentre writes
 *      them.  With |sx| >= W or |sy| >= W every cell leaves and every cell enters.
 * Invariant.  The WORLD VIEW V is the canvas with the window laid over it: V[cy][cx] = L[cy - wy][cx - wx]
 * where that is a window cell, canvas[cy][cx] elsewhere.  This call leaves V unchanged at every canvas
 * cell: a cell that leaves takes its value to the place where V showed it, a cell that enters brings
 * the value V showed.
 *
 * lslam_grid_page_flush: canvas[wy + y][wx + x] = logodds[y][x] for every window cell on the canvas;
 * after it the canvas IS the world view.  The window and win are read only; moved[r] = (cells stored, 0).
 * lslam_grid_page_load, the reverse: logodds[y][x] = canvas[wy + y][wx + x] where (x, y) is on the canvas,
 * 0 elsewhere; the canvas and win are read only; moved[r] = (0, cells loaded).  It starts a robot in a
 * stored map.  Neither touches pg.flags (it may be NULL for them).
 *
 * The canvas as a grid: a reader given canvas as logodds, canvas_w as grid_w and the origin
 * origin - win cell sees the world view (after a flush).  That origin is constant while origin moves
 * by multiples of cell that FP64 holds exactly: the caveat of step 3 of lslam_grid_recentre.
 * The canvas costs 2 Cw Cw bytes a robot: 8 MiB at 2048, 32 GiB for 4096 robots.  It does not grow;
 * what leaves it is lost.
 * canvas must not overlap logodds (LSLAM_ERR_ARG).  All three run on the context's main stream, after
 * every earlier call and before every later one, with no host synchronisation inside.  Out-of-range
 * parameters and missing pointers return LSLAM_ERR_ARG (the message names the field), checked before
 * the context is touched; n_robots == 0 does nothing. */
int lslam_grid_recentre_paged(lslam_ctx *ctx, const lslam_recentre_batch *b, const lslam_page_batch *pg,
                              const lslam_grid_params *g, const lslam_recentre_params *p, const lslam_page_params *pp);
int lslam_grid_page_flush(lslam_ctx *ctx, const lslam_page_batch *pg, const int16_t *logodds, const lslam_grid_params *g,
                          const lslam_page_params *pp);
int lslam_grid_page_load(lslam_ctx *ctx, const lslam_page_batch *pg, int16_t *logodds, const lslam_grid_params *g,
                         const lslam_page_params *pp);

/* Distance field: for every cell of every robot's grid, the squared Euclidean distance, in cells, to
 * the nearest source cell, saturated: the clearance of a planner, the likelihood field of a scorer.
 * The grid's geometry is g's grid_w alone, W = grid_w (g is checked as lslam_grid_update checks it).
 * All integers; cap = d_max d_max.  Per robot r:
 *   0. sources.  LSLAM_DIST_OCC: cell (x, y) is a source iff L[y][x] >= occ_min.  LSLAM_DIST_NOT_FREE:
 *      iff L[y][x] > free_max, and every cell off the map is a source too (unknown space is an
 *      obstacle to a planner).  L is read as the 16-bit value it holds, clamped or not.
 *   1. d2[y][x] = min(cap, min over source cells (x', y') of (x - x')^2 + (y - y')^2).  A source cell
 *      has d2 = 0.  The sources off the map of NOT_FREE amount to the minimum with b b,
 *      b = min(x + 1, W - x, y + 1, W - y).
 *   2. n_src[r] = the source cells on the map; flags[r] = LSLAM_DIST_EMPTY iff n_src[r] = 0, else 0.
 *      An EMPTY map gives cap everywhere in OCC mode and min(cap, b b) in NOT_FREE mode.
 * Every cell of d2 is written on every call; logodds is read only.  d2 must not overlap logodds
 * (LSLAM_ERR_ARG).  The field is recomputed whole: there is no incremental update after a revolution.
 * The transform is separable (a column pass g[y][x] = distance to the nearest source of column x
 * saturated at d_max, then d2[y][x] = min over |x - x'| < d_max of (x - x')^2 + g[y][x']^2); the
 * result is integers, so every correct form gives these bits.  The kernel keeps g in LDS
 * (lslam_dist.h); a grid_w above 1757 with a d_max its bitmap cannot hold (grid_w 2048: above 205)
 * returns LSLAM_ERR_UNSUPPORTED.
 * Runs on the context's main stream, after every earlier call: it sees the grid of a preceding
 * lslam_grid_update or lslam_grid_recentre.  Out-of-range parameters and missing pointers return
 * LSLAM_ERR_ARG (the message names the field), checked before the context is touched;
 * n_robots == 0 does nothing. */
int lslam_grid_distance(lslam_ctx *ctx, const lslam_dist_batch *b, const lslam_grid_params *g,
                        const lslam_dist_params *p);

/* The field read under a revolution: one revolution per robot, the robot's pose and its distance
 * field -> how far the revolution's returns lie from the map's sources, and the robot's own
 * clearance.  The grid's geometry is g's cell, grid_w and max_range.  Per robot r:
 *   0. pose, rotation and robot cell: step 0 of lslam_grid_update, verbatim; (c, s) go to rot[r]
 *      (always) and the written bits are the definition's input.  A bad pose (that step's condition)
 *      gives flags[r] = LSLAM_FIELD_BAD_POSE, stats[r] all zero and clear2[r] = 0.  Otherwise
 *      flags[r] = 0 and clear2[r] = d2[Y0][X0], or off2 if the robot cell (X0, Y0) is off the map.
 *   1. points: step 1 of lslam_grid_update, verbatim: a valid point (both coordinates finite, not
 *      exactly (0, 0)) that is not beyond (x x + y y > max_range max_range) has the hit cell (X1, Y1).
 *      v = d2[Y1][X1] on the map, off2 off it.
 *   2. stats[r] = (sum of min(v, trunc2), points scored, points with v <= near2, points whose hit
 *      cell is off the map), over those points: integers, so the order of accumulation does not
 *      matter.
 * cell sqrt(clear2) is the robot's clearance; stats[2] / stats[1] the share of returns on the map's
 * sources; stats[0] / stats[1] the mean truncated squared distance, the beam-end-point score.
 * pose may alias the filter's ukf_x.  Runs on the context's main stream, after every earlier call.
 * Out-of-range parameters and missing pointers return LSLAM_ERR_ARG (the message names the field),
 * checked before the context is touched; n_robots == 0 does nothing. */
int lslam_field_score(lslam_ctx *ctx, const lslam_fieldscore_batch *b, const lslam_grid_params *g,
                      const lslam_fieldscore_params *p);

/* Gauss-Newton pose refinement in the distance field: one revolution per robot, a pose guess and the
 * robot's field -> the pose nearby at which the revolution's returns lie closest to the map's sources,
 * by at most n_iter damped Gauss-Newton steps on the bilinearly interpolated field, and the normal
 * equations of the alignment there.  A tracker's step (a few descents from the filter's pose); the
 * correlative matchers and the relocaliser serve a robot that has lost track.  The grid's geometry is
 * g's cell, grid_w and max_range (g is checked as lslam_grid_update checks it), W = grid_w,
 * inv = 1.0 / cell, S = 20.  Per robot r, in FP64 with every operation rounded on its own (nothing is
 * fused), then integers:
 *   0. pose.  (px, py, theta) = pose[r], the guess.  A bad pose is step 0 of lslam_grid_update, verbatim
 *      (a non-finite pose component or origin, or |X0d| or |Y0d| >= 2^20): flags[r] =
 *      LSLAM_FIELDALIGN_BAD_POSE, pose_out[r] = pose[r] bit for bit, and trace, normal, n_used and iters
 *      of the robot are zeros.
 *   1. evaluation k = 0, 1, .. at the pose (px, py, theta) as it then stands.  (c, s) = the library's
 *      cos and sin of theta; trace[r][k] = (px, py, theta, c, s), and the written bits of (c, s) are the
 *      definition's input.  The points are those of lslam_grid_update steps 0-1: valid (both
 *      coordinates finite, not exactly (0, 0)) and not beyond (x x + y y > max_range max_range); their
 *      count, the same at every evaluation, is n_valid.  For each of them:
 *        rx = c x - s y, ry = s x + c y, wx = px + rx, wy = py + ry;
 *        u = (wx - ox) inv - 0.5, iu = floor(u), fu = u - iu; v = (wy - oy) inv - 0.5, iv = floor(v),
 *        fv = v - iv: a field value belongs to the centre of its cell.  The point is skipped unless
 *        0 <= iu <= W - 2 and 0 <= iv <= W - 2 (compared as doubles; a NaN fails): all four corners
 *        (ix .. ix + 1, iy .. iy + 1), (ix, iy) = (iu, iv) as integers, lie on the map.
 *        A corner's distance is dq(w) = (double)isqrt(65536 w) / 256.0 with the INTEGER square root
 *        (floor), exact whatever a hardware square root rounds to: d00 = dq(d2[iy][ix]),
 *        d10 = dq(d2[iy][ix + 1]), d01 = dq(d2[iy + 1][ix]), d11 = dq(d2[iy + 1][ix + 1]).
 *        e0 = d10 - d00, e1 = d11 - d01, a0 = d00 + fu e0, a1 = d01 + fu e1, gy = a1 - a0,
 *        m = a0 + fv gy, gx = e0 + fv (e1 - e0): the interpolated distance and its two partial
 *        derivatives, in cells and cells per cell.  jt = (gy rx - gx ry) inv, its derivative by theta.
 *        The point is skipped if m > trunc: an outlier costs nothing.  Otherwise it is used, and its
 *        ten terms are, in this order, gx gx, gx gy, gx jt, gy gy, gy jt, jt jt, gx m, gy m, jt m, m m;
 *        each term t is the int64 rint(t 2^S), round-half-even (the product by 2^S is exact).
 *      N[0..9] = the sums of the ten terms over the used points, as integers: the order of lanes and
 *      waves does not matter.  n_k = the number of used points.
 *      Overflow: the field min(d, d_max) is 1-Lipschitz between neighbouring cells and dq floors it to
 *      a multiple of 1/256, so |gx|, |gy| <= 1 + 1/256; max_range / cell <= 4096 bounds the lever arm,
 *      |jt| <= (1 + 1/256) sqrt(2) 4096 < 5817; m <= trunc <= 255.  The largest term, jt jt 2^S, is
 *      below 2^45.02, so the sums of up to 2^16 = 65536 points per robot stay below 2^61.1, inside
 *      int64, and S = 20 stands.  A robot with more points than that is not supported.
 *      If n_k < min_points: LSLAM_FIELDALIGN_FEW, and the iteration ends here.  If k = n_iter, or the
 *      step before this evaluation set CONVERGED, the iteration ends here: this is the evaluation after
 *      the last step.
 *   2. step k (k < n_iter).  sc = 2^-S.  H00 = (double)N0 sc + damp_t, H01 = (double)N1 sc,
 *      H02 = (double)N2 sc, H11 = (double)N3 sc + damp_t, H12 = (double)N4 sc, H22 = (double)N5 sc +
 *      damp_r, g0 = (double)N6 sc, g1 = (double)N7 sc, g2 = (double)N8 sc (the conversions round to
 *      nearest even).  LDL^T, a pivot being good iff it is > 0 and finite:
 *        d0 = H00; l10 = H01 / d0, l20 = H02 / d0; d1 = H11 - l10 H01; t21 = H12 - l20 H01,
 *        l21 = t21 / d1; d2 = (H22 - l20 H02) - l21 t21;
 *        y0 = g0, y1 = g1 - l10 y0, y2 = (g2 - l20 y0) - l21 y1; z0 = y0 / d0, z1 = y1 / d1, z2 = y2 / d2;
 *        x2 = z2, x1 = z1 - l21 x2, x0 = (z0 - l10 x1) - l20 x2; (dx, dy, dt) = (-x0, -x1, -x2),
 *      dx and dy in cells, dt in rad: the solution of (J^T J + diag(damp_t, damp_t, damp_r)) delta =
 *      -J^T r.  With positive damping the system is positive definite even in a corridor, and the
 *      direction that the revolution does not observe does not move.  The stepped pose is
 *      (px + dx cell, py + dy cell, theta + dt), no angle wrap.  If a pivot is bad (the pivots are
 *      tested in order; the first bad one ends the solve) or a component of the stepped pose is not
 *      finite: LSLAM_FIELDALIGN_SINGULAR, the pose stays, and the iteration ends here.  Otherwise the
 *      pose becomes the stepped pose, iters[r] = k + 1, and LSLAM_FIELDALIGN_CONVERGED is set iff
 *      max(|dx|, |dy|) < eps_t and |dt| < eps_r.  Evaluation k + 1 follows.
 *   3. gates, on the pose (px, py, theta) as it stands at the end and the guess (px0, py0, theta0):
 *      LSLAM_FIELDALIGN_DIVERGED iff |px - px0| > max_shift or |py - py0| > max_shift or
 *      |theta - theta0| > max_turn; LSLAM_FIELDALIGN_WEAK iff 1000 n_last < min_permille n_valid (int64),
 *      n_last the used points of the last evaluation made.
 *   4. outputs.  pose_out[r] = the pose at the end, unless one of BAD_POSE, SINGULAR, FEW, DIVERGED,
 *      WEAK is set: then pose[r] bit for bit (copied as 64-bit words).  normal[r] = N of the last
 *      evaluation made; n_used[r] = (n_0, n_last, n_valid); iters[r]; flags[r]; rows of trace[r] beyond
 *      the last evaluation made are zeros.  Everything but pose_out is reported as computed whatever
 *      the flags.
 * An EMPTY field has no gradient: every step is exactly zero, and CONVERGED comes with the first (if
 * d_max <= trunc; otherwise every point is skipped).  H = normal[0..5] 2^-S and g = normal[6..8] 2^-S
 * are the Gauss-Newton information matrix and vector of the alignment at pose_out, in cells and rad.
 * pose_out may be pose (the filter's ukf_x): the one thread that writes a robot's outputs belongs to
 * the one wave that read its pose, and writes after it (lslam_map_match step 5's rule).  The whole
 * iteration is one launch (lslam_fieldalign.h).  Runs on the context's main stream, after every
 * earlier call: it sees the field of a preceding lslam_grid_distance and the origin of a preceding
 * lslam_grid_recentre.  Out-of-range parameters and missing pointers return LSLAM_ERR_ARG (the message
 * names the field), checked before the context is touched; n_robots == 0 does nothing. */
int lslam_field_align(lslam_ctx *ctx, const lslam_fieldalign_batch *b, const lslam_grid_params *g,
                      const lslam_fieldalign_params *p);

/* Field fusion: lslam_field_align as a measurement update of the filter.  The aligned pose is taken as a
 * measurement z of the pose, with an information matrix built from the alignment's own normal equations,
 * and (x, P) = (a.pose, P) is updated by a Kalman step in information form, gated on the innovation
 * under the filter's own uncertainty.  The information form is deliberate: the undamped J^T J is singular
 * in a corridor, so that a covariance R = inverse(Lambda) does not exist there; every quantity below is
 * built from products and inverses of positive definite sums, and no two nearly equal matrices are
 * subtracted.  All arithmetic is FP64, every operation rounded on its own.  Every element of a 3 x 3
 * product is (t0 + t1) + t2.  "inverse" is the adjugate/determinant form of lslam_map_fuse step 7: the
 * same nine entries p q - r s, det = (S00 A00 + S01 A10) + S02 A20, Si_ij = A_ij / det, and it passes iff
 * S00 > 0 and A22 > 0 and det > 0 and det finite.  cell is g's, inv = 1.0 / cell.  Per robot r:
 *   0-4. steps 0-4 of lslam_field_align, verbatim, with b->a, g and p, but that the pose which step 4
 *      writes to pose_out goes to z[r] (for a rejected robot the guess, bit for bit).  trace, normal,
 *      n_used, iters and flags are written as that call writes them.
 *   5. if any of BAD_POSE, SINGULAR, FEW, DIVERGED, WEAK is set: info, info_f, s2 and nis are zeros,
 *      pose_out and P_out are pose and P bit for bit (copied as 64-bit words: a NaN keeps its payload),
 *      and the steps below are skipped.
 *   6. noise.  n = n_last, sc = 2^-20, N = normal[r].  mean = ((double)N9 sc) / (double)n, or 0.0 if
 *      n = 0; s2 = fmax(mean, sigma_min sigma_min) r_scale: the mean squared residual of the last
 *      evaluation, in squared cells, floored and scaled.
 *   7. the alignment's information, in mm and rad.  u = (inv, inv, 1.0).  For i <= j, k the index of
 *      (xx, xy, xt, yy, yt, tt): Lambda_ij = ((((double)Nk sc) u_i) u_j) / s2, Lambda_ji = Lambda_ij.
 *      There is no damping.  info[r] = Lambda.
 *   8. floor.  ft = (floor_t cell)(floor_t cell), fr = floor_r floor_r, w = (1.0 / ft, 1.0 / ft,
 *      1.0 / fr), taken once per call.  B = Lambda + diag(w) (three additions), Bi = inverse(B),
 *      T = Lambda Bi, E_ij = T_ij w_j, Lambda_f = 0.5 (E_ij + E_ji): the information of the alignment's
 *      covariance plus diag(ft, ft, fr), exact where a row of Lambda is zero.  info_f[r] = Lambda_f; if
 *      B's inverse fails its test, info_f[r] is zeros.
 *   9. prior.  Pi = inverse(P), M_ij = Pi_ij + Lambda_f_ij, Mi = inverse(M), Po_ij = 0.5 (Mi_ij + Mi_ji).
 *      LSLAM_FIELDFUSE_BAD_COV iff some entry of P is not finite, or one of the three inverses fails its
 *      test, or a diagonal entry of Po is not finite and > 0; then nis = 0.0 and steps 10-11 are skipped.
 *   10. innovation and gate.  y_i = z_i - x_i, b = Lambda_f y, c = Po b, e = Pi c,
 *      nis = (y0 e0 + y1 e1) + y2 e2: y^T inverse(P + R) y in product form.  LSLAM_FIELDFUSE_OUTLIER iff
 *      not (nis <= nis_max).
 *   11. update, iff neither BAD_COV nor OUTLIER: pose_out_i = x_i + c_i (no angle wrap), P_out = Po.
 *      Otherwise pose_out and P_out are the input bits.  z, info, info_f, s2 and nis are reported as
 *      computed.
 * The field was drawn from the filter's own poses, so z is not independent of x: r_scale is the knob for
 * that.  The residuals of points that share field cells are not independent either: the floors stand in
 * for that.  z must not overlap a.pose, a.pose_out, P or P_out (LSLAM_ERR_ARG).  a.pose_out may be a.pose
 * and P_out may be P: the one thread that writes a robot's pose_out and P_out has read its pose and P
 * first.  The alignment is fieldalign_kernel's launch; steps 5-11 are one more launch on the same stream,
 * one thread per robot (lslam_fieldfuse.h).  Runs on the context's main stream, after every earlier call.
 * p is checked as lslam_field_align checks it.  Out-of-range parameters and missing pointers return
 * LSLAM_ERR_ARG (the message names the field), checked before the context is touched; n_robots == 0
 * does nothing. */
int lslam_field_fuse(lslam_ctx *ctx, const lslam_fieldfuse_batch *b, const lslam_grid_params *g,
                     const lslam_fieldalign_params *p, const lslam_fieldfuse_params *f);

/* Relocalisation with priors: lslam_map_relocalize over a set of admissible coarse candidates, the cells
 * where the clearance field says a robot can stand and the cells and headings of a window around a stale
 * pose.  A candidate outside the set scores 0 and is not searched.  b->r, g, m and q are checked as
 * lslam_map_relocalize checks them, pp as its table says.  Per robot r it is steps 0-6 of
 * lslam_map_relocalize, verbatim, with b->r, but for the following; f, Wc, cellc as there, (ox, oy) the
 * robot's origin, (wx, wy, wtheta) = win_pose[r]:
 *   field admissibility: Af[ty][tx] = 1 iff some fine cell of the f x f block of coarse cell (ty, tx) has
 *      clear_d2 >= clear_min2; all ones if clear_d2 is NULL.  The rule is lenient on purpose: the fine
 *      stage moves the pose inside the block, and step 5' is the strict test.
 *   window admissibility: cx = ox + ((double)tx + 0.5) cellc, cy = oy + ((double)ty + 0.5) cellc
 *      (cand_pose's own expressions).  Aw[ty][tx] = 1 iff fabs(cx - wx) <= half_xy and
 *      fabs(cy - wy) <= half_xy.  H[k] = 1 iff fabs(remainder((double)k head_step - wtheta,
 *      6.283185307179586)) <= half_theta, remainder being the IEEE operation (exact).  With win_pose NULL,
 *      Aw and H are all ones.  A NaN in win_pose makes its comparisons false: nothing is admissible, and
 *      the robot ends LOST by the rules below, with no special case.
 *   counts: n_admit[r] = (the number of cells with Af & Aw, the number of k with H).
 *   2'. Sc'[k][ty][tx] = Sc[k][ty][tx] where Af & Aw & H[k], else 0.  Step 3 runs on Sc' unchanged: a peak
 *      needs a score > 0 and a 0 never comes before a positive candidate, so an inadmissible cell is
 *      never a candidate and never suppresses one.  coarse_scores, if given, receives Sc'.
 *   5'. fine_clear2[j][r]: with (X0, Y0) the cell of fine_pose[j] by step 0 of lslam_grid_update (as
 *      lslam_field_score takes clear2), clear_d2[Y0][X0]; -1 where that step calls the pose bad (a missing
 *      rank's NaNs are) or the cell is off the map; 0 everywhere if clear_d2 is NULL.  Rank j is eligible
 *      iff step 5's rule holds and, when clear_d2 is given, fine_clear2[j][r] >= clear_min2.
 * Preconditions the call cannot check: clear_d2 is the LSLAM_DIST_NOT_FREE field of the same logodds,
 * computed with d_max d_max >= clear_min2.  clear_d2 must overlap no output (LSLAM_ERR_ARG).
 * Identity: with clear_d2 and win_pose both NULL every output of b->r equals lslam_map_relocalize's bit
 * for bit.  No result depends on the chunking of lslam_set_reloc_budget.  The admissible set is built
 * once per robot (a bit per coarse cell, a list of headings); the search then runs only over the spans
 * of 32 cells that hold an admissible one and over the admissible headings (lslam_relocprior.h).  Runs on
 * the context's main stream, under LSLAM_K_RELOC.  Out-of-range parameters and missing pointers return
 * LSLAM_ERR_ARG (the message names the field), checked before the context is touched; n_robots == 0
 * does nothing. */
int lslam_map_relocalize_prior(lslam_ctx *ctx, const lslam_relocprior_batch *b, const lslam_grid_params *g,
                               const lslam_mapmatch_params *m, const lslam_reloc_params *q,
                               const lslam_relocprior_params *pp);

/* ---- map merge (lslam_grid_merge): modes (lslam_gridmerge_params.mode) and flags (lslam_gridmerge_batch.flags) ---- */
enum {
    LSLAM_MERGE_ADD = 0,      /* the source's evidence is added: L' = clip(L + v) where v != 0 */
    LSLAM_MERGE_FILL = 1      /* the source fills what the destination does not know: L' = clip(v) where L = 0 != v */
};
enum {
    LSLAM_MERGE_MERGED = 1,    /* the destination took the source's evidence */
    LSLAM_MERGE_WEAK = 2,      /* supported < min_support: too little common wall to judge the transform */
    LSLAM_MERGE_CONFLICT = 4,  /* the contradicted share of the source's occupied cells is above max_contra_permille */
    LSLAM_MERGE_SKIPPED = 8,   /* src_index outside 0..n_src-1: the pair does nothing */
    LSLAM_MERGE_BAD_XFORM = 16 /* a component of xform or of an origin is not finite: the pair does nothing */
};

/* Map merge (lslam_grid_merge), 32 bytes.  The destination's geometry (grid_w, cell) and the clamps
 * (l_min, l_max) come from the lslam_grid_params given with the call. */
typedef struct lslam_gridmerge_params {
    int32_t src_w;               /* cells a side of every source grid; 16..2048 (512).  It may differ from grid_w */
    int32_t n_src;               /* source grids at src; >= 1 (1) */
    int32_t occ_min;             /* a cell with L >= occ_min is occupied; -32768..32767 (85) */
    int32_t mode;                /* LSLAM_MERGE_ADD (0) or LSLAM_MERGE_FILL */
    int32_t dry_run;             /* 0 or 1: statistics and flags only (0) */
    int32_t min_support;         /* gate: supported cells a merge needs; >= 0 (64) */
    int32_t max_contra_permille; /* gate: most contradicted cells per 1000 supported or contradicted; 0..1000 (100) */
    int32_t reserved;
} lslam_gridmerge_params;

/* One merge per pair, 72 bytes; all pointers DEVICE memory; all required but src_index. */
typedef struct lslam_gridmerge_batch {
    int32_t n_pairs;
    int32_t reserved;
    const int16_t *src;        /* [n_src][src_w][src_w], row Y: read only, must not overlap dst */
    const double *src_origin;  /* [n_src][2] world coordinates (source frame) of the corner of source cell (0, 0) */
    const int32_t *src_index;  /* [n_pairs], optional (NULL: pair m reads source m) */
    int16_t *dst;              /* [n_pairs][grid_w][grid_w] in/out, row Y */
    const double *dst_origin;  /* [n_pairs][2] */
    const double *xform;       /* [n_pairs][4] (c, s, tx, ty): destination world -> source world */
    int32_t *stats;            /* [n_pairs][8] */
    int32_t *flags;            /* [n_pairs] LSLAM_MERGE_* */
} lslam_gridmerge_batch;

/* lslam_abi_sizes for lslam_gridmerge_params, lslam_gridmerge_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_gridmerge_abi_sizes(int64_t *sizes, int n);
int lslam_gridmerge_params_default(lslam_gridmerge_params *p);

/* Map merge: fold one map into another under a rigid transform, gated on their agreement.  Pair m reads
 * source grid k = src_index[m] (m if src_index is NULL) and changes destination grid m.  The
 * destination's geometry is g's grid_w and cell, W = grid_w, inv = 1.0 / cell; the source's is src_w
 * (Sw) and the same cell.  xform[m] = (c, s, tx, ty) takes destination-world coordinates to
 * source-world coordinates; its bits are the caller's (mapping.merge_transform in Python): there is no
 * trigonometry in the library.  All FP64, every operation rounded on its own (nothing is fused), then
 * integers.  Per pair m:
 *   0. k outside 0..n_src-1: flags[m] = LSLAM_MERGE_SKIPPED, stats[m] all zero, nothing else happens.
 *   1. if any of c, s, tx, ty, dst_origin[m] = (oxd, oyd), src_origin[k] = (oxs, oys) is not finite:
 *      flags[m] = LSLAM_MERGE_BAD_XFORM, stats[m] all zero, nothing else happens.
 *   2. the gather.  For destination cell (X, Y): wx = oxd + ((double)X + 0.5) cell, wy = oyd +
 *      ((double)Y + 0.5) cell; xs = (c wx - s wy) + tx, ys = (s wx + c wy) + ty;
 *      fx = floor((xs - oxs) inv), fy = floor((ys - oys) inv).  The cell is ON THE SOURCE MAP iff
 *      0 <= fx < Sw and 0 <= fy < Sw, compared as doubles before any conversion (a NaN fails, so a
 *      transform at 1e300 converts nothing).  v = src[k][fy][fx] there, 0 elsewhere: an inverse
 *      nearest-neighbour gather, every destination cell decided exactly once, no holes under rotation.
 *   3. classes, against the destination L as it stood before the call.  N(X, Y) iff some cell of the
 *      3 x 3 block around (X, Y), clipped to the map, has L >= occ_min.  A cell with v >= occ_min is
 *      SUPPORTED if N(X, Y); CONTRADICTED if not N(X, Y) and L[Y][X] < 0; NEW otherwise.
 *      stats[m] = (cells on the source map, cells with v != 0, supported, contradicted, new, cells with
 *      L != 0 != v of equal sign, cells with L != 0 != v of opposite sign, cells whose value changed).
 *   4. gates.  LSLAM_MERGE_WEAK iff supported < min_support.  LSLAM_MERGE_CONFLICT iff
 *      1000 contradicted > max_contra_permille (supported + contradicted), in 64 bits.  Either gate, or
 *      dry_run, leaves dst bit for bit and the changed count 0; flags[m] = the gates that are set (0: a
 *      dry run that would have merged).
 *   5. otherwise flags[m] = LSLAM_MERGE_MERGED and, with l_min and l_max of g:
 *      ADD:  where v != 0, L' = clip(L + v, l_min, l_max) (the sum in 32 bits);
 *      FILL: where L = 0 and v != 0, L' = clip(v, l_min, l_max).
 *      Every other cell keeps its bits, values outside [l_min, l_max] included.  The changed count is
 *      the cells with L' != L.
 * ADD counts evidence twice when the same source is merged twice; FILL does not.  The gates read
 * occupied cells only: two maps without a common occupied cell merge WEAK.  The resampling is nearest
 * neighbour: under rotation a one-cell wall may come out one cell off or doubled, which is what the
 * one-cell tolerance of N is for.
 * Two launches on the main stream (lslam_gridmerge.h): the statistics, then the merge, every workgroup
 * of which takes the pair's decision from the finished counters; stats is the only scratch.  src must
 * not overlap dst (LSLAM_ERR_ARG).  Runs on the context's main stream, after every earlier call, with
 * no host synchronisation inside; there is no timing slot.  g is checked as lslam_grid_update checks
 * it.  Out-of-range parameters and missing pointers return LSLAM_ERR_ARG (the message names the field),
 * checked before the context is touched; n_pairs == 0 does nothing. */
int lslam_grid_merge(lslam_ctx *ctx, const lslam_gridmerge_batch *b, const lslam_grid_params *g,
                     const lslam_gridmerge_params *p);

/* ---- a map as a revolution (lslam_grid_points): flags (lslam_gridpoints_batch.flags) ---- */
enum {
    LSLAM_GRIDPOINTS_BAD_ANCHOR = 1, /* a component of anchor or of origin is not finite: no point */
    LSLAM_GRIDPOINTS_EMPTY = 2,      /* no occupied cell in range: n_out = 0 */
    LSLAM_GRIDPOINTS_DECIMATED = 4   /* more occupied cells in range than slots: every stride-th was taken */
};
/* bands of rows that a grid is cut into at most: the second dimension of lslam_gridpoints_batch.band_counts */
#define LSLAM_GRIDPOINTS_BANDS 256

/* A map as a revolution (lslam_grid_points), 16 bytes (a multiple of 8 as it stands: no reserved field).
 * The grid's geometry (grid_w, cell) comes from the lslam_grid_params given with the call. */
typedef struct lslam_gridpoints_params {
    double radius;   /* mm: cells whose centre is further from the anchor are left out; > 0 and finite (8000.0) */
    int32_t occ_min; /* a cell with L >= occ_min is occupied; -32768..32767 (85) */
    int32_t cap;     /* slots per robot; 1..65536 (1024) */
} lslam_gridpoints_params;

/* One point set per robot, 72 bytes; all pointers DEVICE memory; all required. */
typedef struct lslam_gridpoints_batch {
    int32_t n_robots;
    int32_t reserved;
    const int16_t *logodds; /* [R][grid_w][grid_w], row Y: read only */
    const double *origin;   /* [R][2] world coordinates of the corner of cell (0, 0) */
    const double *anchor;   /* [R][4] (ax, ay, c, s): the anchor pose's position in the map's world frame, cos and sin of its heading */
    double *xy;             /* [R][cap][2]: the points in the anchor's frame, (+0.0, +0.0) behind the last */
    int32_t *pt_off;        /* [R + 1]: r * cap */
    int32_t *counts;        /* [R][4] (n_occ, n_in, stride, n_out) */
    int32_t *flags;         /* [R] LSLAM_GRIDPOINTS_* */
    int32_t *band_counts;   /* [R][LSLAM_GRIDPOINTS_BANDS][2]: scratch, the count pass's (n_occ, n_in) per band */
} lslam_gridpoints_batch;

/* lslam_abi_sizes for lslam_gridpoints_params, lslam_gridpoints_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_gridpoints_abi_sizes(int64_t *sizes, int n);
int lslam_gridpoints_params_default(lslam_gridpoints_params *p);

/* A map as a revolution: the occupied cells of each robot's grid within radius of an anchor pose, as
 * points in that pose's frame, in the CSR revolution form that lslam_map_relocalize, lslam_map_match,
 * lslam_field_score, lslam_field_align and lslam_grid_raycast read (xy, pt_off): what a stored map, a
 * canvas or a map whose robot has gone offers in place of a revolution.  anchor[r] = (ax, ay, c, s): the
 * bits of c = cos theta and s = sin theta are the caller's; there is no trigonometry in the library.
 * W = grid_w and cell are g's.  All FP64, every operation rounded on its own (nothing is fused), then
 * integers; r2 = radius * radius, one product taken on the host.  Per robot r:
 *   0. pt_off[r] = r * cap for r in 0..R, always (R * cap >= 2^31 is refused: LSLAM_ERR_ARG).
 *   1. if any of ax, ay, c, s, origin[r] = (ox, oy) is not finite: flags[r] = LSLAM_GRIDPOINTS_BAD_ANCHOR,
 *      counts[r] all zero, every slot of robot r is (+0.0, +0.0); nothing else happens.
 *   2. the cells in row-major order, Y outer, X inner.  A cell is occupied iff L[Y][X] >= occ_min.
 *      wx = ox + ((double)X + 0.5) cell, wy = oy + ((double)Y + 0.5) cell; dx = wx - ax, dy = wy - ay;
 *      d2 = dx dx + dy dy.  An occupied cell is IN RANGE iff d2 > 0.0 and d2 <= r2 (the cell whose centre
 *      is the anchor is left out: (0, 0) is the matchers' invalid point).  i is the cell's ordinal among
 *      the occupied cells in range; n_occ counts the occupied cells, n_in those in range.
 *   3. stride = max(1, (n_in + cap - 1) / cap).  Cell i is taken iff i % stride == 0, into slot
 *      j = i / stride; n_out = (n_in + stride - 1) / stride <= cap.
 *   4. xy[r][j] = ((c dx) + (s dy), (c dy) - (s dx)).  Slots n_out..cap-1 are (+0.0, +0.0): every consumer
 *      that uses the scan matcher's validity rule skips them.
 *   5. counts[r] = (n_occ, n_in, stride, n_out); flags[r] = LSLAM_GRIDPOINTS_EMPTY iff n_out == 0, else
 *      LSLAM_GRIDPOINTS_DECIMATED iff stride > 1, else 0.
 * The slots are fixed (robot r owns xy[r * cap .. (r + 1) * cap)), so the host knows pt_off without
 * waiting for the device.  Decimation by stride follows the row-major order: it is not uniform in
 * space, and a thick wall weighs more than a thin one.  A map seen as a scan has no occlusion.
 * Two launches on the main stream behind a memset of xy (lslam_gridpoints.h): the count pass writes
 * (n_occ, n_in) of every band of rows to band_counts, the caller's scratch (2 KiB a robot: the context
 * holds none for this call, so nothing grows and nothing waits); the write pass takes each band's first
 * ordinal from the finished counts and stores the taken points in order, without atomics.  Nothing is
 * written beyond xy[R * cap], pt_off[R + 1], counts[R][4], flags[R] and band_counts.  Runs on the
 * context's main stream, after every earlier call, with no host synchronisation inside; there is no
 * timing slot.  g is checked as lslam_grid_update checks it.  Out-of-range parameters and missing
 * pointers return LSLAM_ERR_ARG (the message names the field), checked before the context is touched;
 * n_robots == 0 does nothing. */
int lslam_grid_points(lslam_ctx *ctx, const lslam_gridpoints_batch *b, const lslam_grid_params *g,
                      const lslam_gridpoints_params *p);

/* ---- pose-graph optimisation (lslam_pose_graph): flags (lslam_posegraph_batch.flags) ---- */
enum {
    LSLAM_POSEGRAPH_EMPTY = 1,     /* fewer than two nodes or no edge: nothing is evaluated, pose_out is pose */
    LSLAM_POSEGRAPH_BAD_GRAPH = 2, /* a count out of range, an edge on a node that is not there, or a value that is not finite: pose_out is pose */
    LSLAM_POSEGRAPH_CONVERGED = 4, /* a step fell below eps_t and eps_r at every node */
    LSLAM_POSEGRAPH_SINGULAR = 8,  /* a pivot of the solve is not finite and > 0, or a stepped pose is not finite: pose_out is pose */
    LSLAM_POSEGRAPH_DIVERGED = 16  /* chi2 of the last evaluation is not <= that of the first: pose_out is pose */
};

/* Pose-graph optimisation (lslam_pose_graph), 48 bytes. */
typedef struct lslam_posegraph_params {
    double damp_t;     /* 1/mm^2, added to the x and y diagonal of every free node; >= 0 and finite (1e-6) */
    double damp_r;     /* 1/rad^2, added to the theta diagonal; >= 0 and finite (1e-3) */
    double eps_t;      /* mm: a step below it at every node (with eps_r) ends the iteration; >= 0 and finite (0.01) */
    double eps_r;      /* rad; >= 0 and finite (1e-5) */
    int32_t max_nodes; /* N_cap: the node dimension of pose, pose_out and trace; 2..64 (48) */
    int32_t max_edges; /* E_cap: the edge dimension of edge_ij, edge_z, edge_info and edge_chi2; 1..1024 (256) */
    int32_t n_iter;    /* Gauss-Newton steps at most; 0..32 (10) */
    int32_t reserved;
} lslam_posegraph_params;

/* One graph per robot, 104 bytes; all pointers DEVICE memory; all required.  pose and pose_out are
 * NODE-MAJOR: slab k is a contiguous [n_graphs][3], what every map-side call takes as its pose. */
typedef struct lslam_posegraph_batch {
    int32_t n_graphs;
    int32_t reserved;
    const int32_t *n_nodes;  /* [G] */
    const int32_t *n_edges;  /* [G] */
    const double *pose;      /* [N_cap][G][3] (x, y in mm, theta in rad) */
    const int32_t *edge_ij;  /* [G][E_cap][2] */
    const double *edge_z;    /* [G][E_cap][3]: the pose of node j in node i's frame */
    const double *edge_info; /* [G][E_cap][6]: the symmetric Omega in i's frame as xx, xy, xt, yy, yt, tt (1/mm^2, 1/(mm rad), 1/rad^2) */
    double *pose_out;        /* [N_cap][G][3]; may be pose */
    double *trace;           /* [G][n_iter + 1][N_cap][2] (cos, sin) of every node at every evaluation, zeros beyond */
    double *chi2;            /* [G][2]: of the first and of the last evaluation */
    double *edge_chi2;       /* [G][E_cap]: per edge at the last evaluation */
    int32_t *iters;          /* [G] steps taken */
    int32_t *flags;          /* [G] LSLAM_POSEGRAPH_* */
} lslam_posegraph_batch;

/* lslam_abi_sizes for lslam_posegraph_params, lslam_posegraph_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_posegraph_abi_sizes(int64_t *sizes, int n);
int lslam_posegraph_params_default(lslam_posegraph_params *p);

/* Pose-graph optimisation: per robot one graph whose nodes are keyframe poses (x, y, theta) and whose
 * edges are relative-pose measurements (odometry between consecutive keyframes, loop closures between
 * distant ones), solved by damped Gauss-Newton with node 0 held as the gauge.  The corrected poses come
 * out node-major, so that a map can be redrawn from them slab by slab (lslam_grid_update).
 * N_cap = max_nodes, E_cap = max_edges.  All FP64, every operation rounded on its own (nothing is
 * fused).  Per graph, N = n_nodes and E = n_edges; x_i = (x_i, y_i, theta_i):
 *   0. Checks.  If N < 0, E < 0, N > N_cap or E > E_cap: LSLAM_POSEGRAPH_BAD_GRAPH.  Else if N < 2 or
 *      E = 0: LSLAM_POSEGRAPH_EMPTY.  Else LSLAM_POSEGRAPH_BAD_GRAPH iff an edge e < E has i = j or an
 *      index outside 0..N-1, or a component of a pose of nodes 0..N-1, of a z or of an Omega of edges
 *      0..E-1 is not finite.  With either flag pose_out = pose bit for bit (all N_cap slabs, copied as
 *      64-bit words), flags is that one flag, and trace, chi2, edge_chi2 and iters of the graph are
 *      zero; nothing else happens.
 *   1. Evaluation k = 0, 1, ... at the poses as they then stand.  (c_i, s_i) = the library's cos and
 *      sin of theta_i, written to trace[g][k][i] for i < N; the written bits are the definition's
 *      input.  Per edge e = (i, j, z, Omega):
 *        dx = x_j - x_i, dy = y_j - y_i; ux = (c_i dx) + (s_i dy), uy = (c_i dy) - (s_i dx);
 *        e0 = ux - z0, e1 = uy - z1, e2 = remainder((theta_j - theta_i) - z2, 6.283185307179586), the
 *        IEEE operation, which is exact;
 *        A = de/dx_i = [[-c, -s, uy], [s, -c, -ux], [+0, +0, -1]],
 *        B = de/dx_j = [[c, s, +0], [-s, c, +0], [+0, +0, 1]];
 *        MA = Omega A, MB = Omega B, w = Omega e, chi_e = e^T w, and the contributions A^T MA to block
 *        (i, i), A^T MB to block (i, j), its transpose bit for bit to (j, i), B^T MB to (j, j), A^T w
 *        to g_i and B^T w to g_j.  Every element of these 3-term products is (t0 + t1) + t2 over the
 *        inner index 0, 1, 2, with all three products formed (the zeros and ones of A and B too).
 *      Every element of the lower triangle of H and of g is the sum, from +0.0, of its contributions in
 *      ascending e; chi2_k is the sum of chi_e from +0.0 in ascending e; edge_chi2[g][e] = chi_e of the
 *      last evaluation made.  The iteration ends here if k = n_iter or the step before set
 *      LSLAM_POSEGRAPH_CONVERGED.
 *   2. Step k.  Node 0's rows and columns are dropped: n = 3 (N - 1) unknowns, node v's at 3 (v - 1).
 *      damp_t, damp_t, damp_r are added to each node's three diagonal elements, after the sums.  LDL^T,
 *      right-looking on the lower triangle: for column p = 0..n-1, d_p = H[p][p] must be > 0 and
 *      finite; l_ap = H[a][p] / d_p for a > p; H[a][b] = H[a][b] - l_ap H[b][p] for p < b <= a, with
 *      H[b][p] the undivided value: one product and one subtraction per p.  Forward: y_a = g_a minus
 *      l_ab y_b, one b at a time in ascending b < a.  z_a = y_a / d_a.  Back: x_a = z_a minus l_ba x_b,
 *      one b at a time in descending b > a.  delta = -x; the stepped pose of a node v >= 1 is
 *      x_v + delta_v, component by component, with no angle wrap; node 0 keeps its bits.  On a pivot
 *      that fails (the first one ends the solve) or a stepped component that is not finite:
 *      LSLAM_POSEGRAPH_SINGULAR, the poses stay, and the iteration ends here.  Otherwise the poses
 *      become the stepped poses, iters = k + 1, and LSLAM_POSEGRAPH_CONVERGED is set iff
 *      |delta| < eps_t for every x and y component and |delta| < eps_r for every theta component.
 *   3. Gate.  LSLAM_POSEGRAPH_DIVERGED iff not (chi2_last <= chi2_0), the last and the first
 *      evaluation made (a NaN fails).
 *   4. Outputs.  pose_out = the poses as they stand for nodes < N, unless LSLAM_POSEGRAPH_SINGULAR or
 *      LSLAM_POSEGRAPH_DIVERGED is set: then pose bit for bit.  The slabs of nodes >= N are copied
 *      through.  chi2 = (chi2_0, chi2_last); trace rows beyond the last evaluation, and the entries of
 *      nodes >= N and of edges >= E, are zeros.
 * z is the pose of j seen from i: z = (R(theta_i)^T (p_j - p_i), theta_j - theta_i), and Omega is the
 * information of that measurement in i's frame.  The solve is dense: 3 (N_cap - 1) <= 189 unknowns in
 * the workgroup's LDS (lslam_posegraph.h), which is what bounds max_nodes.  The solve has no robust kernel:
 * a false closure that reaches it pulls the whole graph (and shows as the largest edge_chi2 only when it
 * is weighted no more strongly than the odometry), so it is rejected before, by lslam_pose_graph_gate.  One launch behind the
 * memsets of trace, chi2, edge_chi2 and iters, one workgroup per graph; only that workgroup reads the
 * graph's pose, and it writes pose_out last, so pose_out may be pose.  Runs on the context's main
 * stream, after every earlier call, with no host synchronisation inside; there is no timing slot.
 * Out-of-range parameters and missing pointers return LSLAM_ERR_ARG (the message names the field),
 * checked before the context is touched; n_graphs == 0 does nothing. */
int lslam_pose_graph(lslam_ctx *ctx, const lslam_posegraph_batch *b, const lslam_posegraph_params *p);

/* ---- closure gating (lslam_pose_graph_gate): a candidate's verdict (lslam_posegate_batch.cand_flags) ---- */
enum {
    LSLAM_POSEGATE_UNJUDGED = 0,  /* no verdict: the slot is beyond n_cand, or the graph is flagged */
    LSLAM_POSEGATE_ACCEPTED = 1,  /* d2 <= nis_max */
    LSLAM_POSEGATE_OUTLIER = 2,   /* not (d2 <= nis_max); a NaN among them */
    LSLAM_POSEGATE_BAD_EDGE = 4,  /* i = j, an index outside 0..N-1, or a z or an Omega that is not finite: nis, err and cov are zero */
    LSLAM_POSEGATE_BAD_INFO = 8,  /* Omega or the innovation covariance has no positive inverse: nis is zero */
    LSLAM_POSEGATE_APPENDED = 16, /* beside ACCEPTED, with append: the candidate is now an edge of the graph */
    LSLAM_POSEGATE_NO_ROOM = 32   /* beside ACCEPTED, with append: the graph already held max_edges edges */
};

/* Closure gating (lslam_pose_graph_gate), 40 bytes. */
typedef struct lslam_posegate_params {
    double damp_t;     /* as lslam_posegraph_params: what the solve that follows will use (1e-6) */
    double damp_r;     /* (1e-3) */
    double nis_max;    /* the gate on d2; > 0, +inf: every candidate with a statistic is accepted (16.27: chi-square, 3 dof, 0.1 %) */
    int32_t max_nodes; /* N_cap: the node dimension of pose and trace; 2..64 (48) */
    int32_t max_edges; /* E_cap: the edge dimension of edge_ij, edge_z and edge_info; 1..1024 (256) */
    int32_t max_cand;  /* C_cap: the candidate dimension of every cand_ array; 1..64 (16) */
    int32_t append;    /* 0: the edge arrays and n_edges are only read; 1: the accepted candidates become edges (0) */
} lslam_posegate_params;

/* One graph per robot and its closure candidates, 144 bytes; all pointers DEVICE memory; all required.  The
 * graph is what lslam_posegraph_batch holds, in that layout, so that the same buffers serve both calls. */
typedef struct lslam_posegate_batch {
    int32_t n_graphs;
    int32_t reserved;
    const int32_t *n_nodes;  /* [G] */
    int32_t *n_edges;        /* [G]; with append also an output */
    const double *pose;      /* [N_cap][G][3] node-major: the poses at which the graph is linearised */
    int32_t *edge_ij;        /* [G][E_cap][2]; with append also an output, as edge_z and edge_info */
    double *edge_z;          /* [G][E_cap][3] */
    double *edge_info;       /* [G][E_cap][6] */
    const int32_t *n_cand;   /* [G] */
    const int32_t *cand_ij;  /* [G][C_cap][2] */
    const double *cand_z;    /* [G][C_cap][3] */
    const double *cand_info; /* [G][C_cap][6] xx, xy, xt, yy, yt, tt */
    double *trace;           /* [G][N_cap][2] (cos, sin) of every node at the evaluation, zeros beyond */
    double *chi2;            /* [G] of the graph at pose, without the candidates */
    double *cand_nis;        /* [G][C_cap] d2 */
    double *cand_err;        /* [G][C_cap][3] e */
    double *cand_cov;        /* [G][C_cap][6] sym(J Sigma J^T) as xx, xy, xt, yy, yt, tt */
    int32_t *cand_flags;     /* [G][C_cap] LSLAM_POSEGATE_* */
    int32_t *flags;          /* [G] 0, LSLAM_POSEGRAPH_EMPTY, LSLAM_POSEGRAPH_BAD_GRAPH or LSLAM_POSEGRAPH_SINGULAR */
} lslam_posegate_batch;

/* lslam_abi_sizes for lslam_posegate_params, lslam_posegate_batch.  Writes min(n, 2) entries, returns 2. */
int lslam_posegate_abi_sizes(int64_t *sizes, int n);
int lslam_posegate_params_default(lslam_posegate_params *p);

/* Closure gating: every candidate edge of a graph is judged, before any solve, against what the graph
 * without it predicts.  With Sigma the covariance of the trusted graph linearised at pose (the inverse of
 * the damped H of lslam_pose_graph) and J the candidate's Jacobian, the statistic is the innovation
 * d2 = e^T (J Sigma J^T + Omega_c^-1)^-1 e, chi-square with three degrees of freedom for a true closure on a
 * calibrated graph: the test lslam_field_fuse applies to a filter measurement.  J Sigma J^T alone, cand_cov,
 * does not depend on z: it is the covariance of where node j is expected in node i's frame, the window in
 * which to look for the closure.  N_cap = max_nodes, E_cap = max_edges, C_cap = max_cand.  All FP64, every
 * operation rounded on its own (nothing is fused), every sum in the order written.  Per graph, N = n_nodes,
 * E = n_edges, C = n_cand:
 *   0. Checks.  LSLAM_POSEGRAPH_BAD_GRAPH if N < 0, E < 0, N > N_cap, E > E_cap, C < 0 or C > C_cap; else
 *      LSLAM_POSEGRAPH_EMPTY if N < 2 or E = 0; else LSLAM_POSEGRAPH_BAD_GRAPH by lslam_pose_graph's test
 *      of the edges 0..E-1 and of the poses 0..N-1.  With either flag every candidate stays
 *      LSLAM_POSEGATE_UNJUDGED, every output of the graph but flags is zero and nothing is appended.
 *   1. One evaluation at pose, bit for bit lslam_pose_graph's step 1: (c_i, s_i) = the library's cos and
 *      sin of theta_i, written to trace[g][i] for i < N (the written bits are the definition's input); H and
 *      g from the edges in ascending e, then damp_t, damp_t, damp_r on every free node's diagonal.
 *      chi2[g] = the sum of chi_e from +0.0 in ascending e: where it is the graph's minimum, pose is the
 *      optimum and Sigma means what it should.
 *   2. The LDL^T of lslam_pose_graph's step 2 on the reduced H (node 0 is the gauge, n = 3 (N - 1)), with
 *      the same element steps.  A pivot that is not finite and > 0 (the first one ends the call for this
 *      graph): LSLAM_POSEGRAPH_SINGULAR; trace and chi2 stay as step 1 wrote them, every candidate stays
 *      LSLAM_POSEGATE_UNJUDGED with zero outputs and nothing is appended.
 *   3. Each candidate c < C = (i, j, z, Omega).  LSLAM_POSEGATE_BAD_EDGE, with zero nis, err and cov, if
 *      i = j, an index is outside 0..N-1, or a component of z or Omega is not finite.  Otherwise e, A and B
 *      of lslam_pose_graph's step 1 at (x_i, x_j, c_i, s_i, z).  R = J^T, n x 3: rows 3 (i - 1).. hold A^T
 *      if i >= 1, rows 3 (j - 1).. hold B^T if j >= 1, every other row is +0.0.  X = H^-1 R, each column
 *      as step 2 of lslam_pose_graph solves for g: forward, divide, back.  M = J X: element (r, k) sums,
 *      from +0.0, A[r][q] X[3 (i - 1) + q][k] over q = 0, 1, 2 if i >= 1, then B[r][q] X[3 (j - 1) + q][k]
 *      likewise if j >= 1 (the gauge contributes nothing).  Ms = 0.5 (M + M^T).  Sc = Omega^-1 and then
 *      Si = (Ms + Sc)^-1, both by the adjugate and the determinant of lslam_map_fuse's step 7 and its pass
 *      test; w = Si e, each element (t0 + t1) + t2; d2 = (e0 w0 + e1 w1) + e2 w2.  cand_err = e and
 *      cand_cov = Ms.  If either inverse fails its test: LSLAM_POSEGATE_BAD_INFO alone and cand_nis = 0.
 *      Otherwise cand_nis = d2, and LSLAM_POSEGATE_ACCEPTED iff d2 <= nis_max (a NaN fails), else
 *      LSLAM_POSEGATE_OUTLIER.  The entries of c >= C are zeros.
 *   4. With append: in ascending c, an ACCEPTED candidate is copied to the edge arrays at index E, E grows
 *      by one and the candidate gains LSLAM_POSEGATE_APPENDED, while E < E_cap; after that it gains
 *      LSLAM_POSEGATE_NO_ROOM.  n_edges[g] = E.  Without append the edge arrays and n_edges are only read.
 * Known limits.  Candidates are judged one by one against the trusted graph, not against each other: two
 * candidates that agree with the graph and contradict one another both pass.  Sigma is the linearised
 * covariance at pose, with the damping in it as a weak prior on every node.  A graph whose odometry
 * information is overconfident rejects true closures.  The solve is still dense, 3 (N_cap - 1) <= 189
 * unknowns in the workgroup's LDS (lslam_posegate.h); a max_nodes, max_edges and max_cand whose LDS does
 * not fit return LSLAM_ERR_UNSUPPORTED.  One launch behind the memsets of every output but flags, one
 * workgroup per graph.  Runs on the context's main stream, after every earlier call, with no host
 * synchronisation inside; there is no timing slot.  Out-of-range parameters and missing pointers return
 * LSLAM_ERR_ARG (the message names the field), checked before the context is touched; n_graphs == 0 does
 * nothing. */
int lslam_pose_graph_gate(lslam_ctx *ctx, const lslam_posegate_batch *b, const lslam_posegate_params *p);

#ifdef __cplusplus
}
#endif
#endif /* LIDARSLAM_H */
