/*
 * pof_abi.h -- C ABI of libpof_hip.so, the MI355X (gfx950) implementation of the
 * per-point planar-flow hot path of huzjkevin/planar_optical_flow.
 *
 * Conventions
 *   - every entry point returns int: POF_OK (0) or a negative POF_E_* code;
 *   - all array arguments are DEVICE pointers owned by the caller; the library
 *     never allocates or frees user-visible memory and keeps no global state
 *     (re-entrant, thread-safe); scratch space is passed in explicitly;
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream);
 *   - shapes are C-contiguous unless a stride argument says otherwise.
 *
 * Each declaration cites the reference interface it replaces (paths relative
 * to the reference checkout).
 */
#ifndef POF_ABI_H
#define POF_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POF_ABI_VERSION 1

enum {
    POF_OK = 0,
    POF_E_BADARG = -1, /* null pointer / illegal enum / negative size          */
    POF_E_SHAPE = -2,  /* sizes inconsistent with each other or with a limit   */
    POF_E_LAUNCH = -3, /* the HIP runtime reported an error on launch          */
    POF_E_WORKSPACE = -4 /* caller workspace too small                         */
};

typedef void *pof_stream_t; /* hipStream_t */

int pof_abi_version(void);
const char *pof_error_string(int code);
/* Every entry point starts from a clean HIP error state (so that its own launch check is meaningful).  A sticky
 * error left by an EARLIER call of the calling thread -- the caller's own previous launch, say -- is not
 * swallowed by that: it is parked, and this function returns it (a hipError_t value; 0 = none) and clears the
 * slot.  Thread-local. */
int pof_take_stale_error(void);

/* ------------------------------------------------------------------------
 * A1  get_laser_phi(angle_inc, num_pts)            src/utils/utils.py:25-29
 * Fills tab[0..N) = phi, tab[N..3N) = (cos phi_i, sin phi_i) interleaved, all
 * float64.  phi is bit-identical to numpy.linspace(-fov/2, fov/2, N).
 * ---------------------------------------------------------------------- */
int pof_laser_phi(double angle_inc, int num_pts, double *tab /* [3*N] */, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A2-A7 fused per-sample preprocessing of the CURRENT scan of each window:
 *   rphi_to_xy                          src/utils/utils.py:47-48
 *   get_displacement_from_odometry      src/utils/utils.py:639-662  (kind 0)
 *   get_flow_target                     src/utils/utils.py:204-229  (kind 1)
 *   get_velocity_from_odometry          src/utils/utils.py:609-636  (kind 2)
 *   data_prepare.get_flow_target        bin/data_prepare.py:29-47   (kind 3; odom0 = odometry
 *                                       difference (dx,dy,dphi), odom1[0] = dt)
 *   scan-pair alignment                 src/utils/dataset.py:76-93  (kind 4; `flow` receives the
 *                                       transformed points; odom0 = (dx,dy,dphi), odom1[0] = scan_dir)
 *   global_to_canonical_flow            src/utils/utils.py:62-75    (canonical != 0)
 *   closest_detection / get_regression_target   src/utils/utils.py:147-185, 232-256
 *   _get_dynamic_mask / _get_valid_point_mask   src/utils/dataset_dr_spaam.py:511-529
 * i.e. the arithmetic of DROWDataset2.__getitem__ (dataset_dr_spaam.py:384-409)
 * for a whole batch in one launch; the collate (dataset_dr_spaam.py:464-471) is
 * implicit because outputs are written in batched layout.
 *
 * ranges        current-scan rows, float32; row b starts at ranges + b*sample_stride
 * tab           output of pof_laser_phi for this N
 * odom0/odom1   [B][3] float64 (x, y, phi); may be NULL when flow and xy are NULL
 * out_f64       0: xy/flow are float32, 1: float64
 * xy, flow      [B][N][2], either may be NULL
 * det_offsets   [B+1] int32 CSR offsets into det_rphi/det_cls, or NULL to skip
 *               association and the dynamic mask
 * det_rphi      [D][2] float64 (r, phi); det_cls [D] uint8 in {0,1,2} = wc, wa, wp
 * assoc_radius  [3] radius per class for closest_detection (reference 0.6,0.4,0.35)
 * labels        [3] class label per class (reference 1,2,3; pedestrian_only: x,x,1)
 * dyn_radius    [3] radius per class for the dynamic mask (reference 2.5,2.0,2.0)
 * closest       [B][N] int64, 1-based detection index within the sample, 0 = none
 * target_cls    [B][N] int64;  target_reg [B][N][2] float32
 * dyn_mask, valid_mask, exclude_mask   [B][N] float32 in {0,1}
 * Any output pointer may be NULL.
 * D             number of rows of det_rphi / det_cls (= det_offsets[B])
 * workspace     device scratch of at least pof_scan_preprocess_workspace_bytes(B, D)
 *               bytes: the per-sample rigid motion and per-detection cartesian
 *               centres (a first, tiny launch) that the streaming launch reads
 *               as wave-uniform scalars.
 * ---------------------------------------------------------------------- */
size_t pof_scan_preprocess_workspace_bytes(int B, int D);
int pof_scan_preprocess(const float *ranges, long long sample_stride, int B, int N,
                        const double *tab, const double *odom0, const double *odom1,
                        int flow_kind, int canonical, int out_f64, void *xy, void *flow,
                        const int32_t *det_offsets, const double *det_rphi, const uint8_t *det_cls,
                        int D, const double *assoc_radius, const int32_t *labels,
                        const double *dyn_radius, int64_t *closest, int64_t *target_cls,
                        float *target_reg, float *dyn_mask, float *valid_mask, float *exclude_mask,
                        void *workspace, size_t workspace_bytes, pof_stream_t stream);

/* Same call split in its two launches, for callers that pipeline independent
 * batches on two streams (params of batch i+1 under the streaming launch of
 * batch i): phases = 1 runs only the per-sample params launch (fills the
 * workspace), phases = 2 only the streaming launch (workspace must have been
 * filled for these inputs), phases = 3 both (= pof_scan_preprocess).
 * Alignment (this call, pof_scan_preprocess and pof_scan_preprocess_chained): none required.  The flat kernel runs
 * when N is even and >= 128, sample_stride is even, ranges is 8-byte and every non-NULL output 16-byte aligned;
 * the same rows with aligned pointers but a short N run 2 points per lane (float2 loads, 16-byte stores), and
 * anything else 1 point per lane with scalar loads and stores.  All three give the same bits, except float32 flow
 * (flow_kind != 1): the flat kernel evaluates it in float32 arithmetic, the per-point kernels round the float64
 * result once, so the last bits may differ (both within 1e-5 m of the float64 reference). */
int pof_scan_preprocess_phase(const float *ranges, long long sample_stride, int B, int N,
                              const double *tab, const double *odom0, const double *odom1,
                              int flow_kind, int canonical, int out_f64, void *xy, void *flow,
                              const int32_t *det_offsets, const double *det_rphi, const uint8_t *det_cls,
                              int D, const double *assoc_radius, const int32_t *labels,
                              const double *dyn_radius, int64_t *closest, int64_t *target_cls,
                              float *target_reg, float *dyn_mask, float *valid_mask, float *exclude_mask,
                              void *workspace, size_t workspace_bytes, int phases, pof_stream_t stream);

/* Chained form for a stream of batches (a data loader knows the next batch):
 * ONE launch streams the current batch -- whose workspace must already hold its
 * params (from the previous chained call, or a phases = 1 call for the first
 * batch) -- and, on extra workgroups of the same grid, evaluates the params of
 * the NEXT batch into next->workspace.  The streaming rows are HBM-bound and
 * leave the ALUs idle, so the next batch's sincos work hides under them and
 * the steady state is one launch per batch.  next == NULL: plain phases = 2. */
typedef struct pof_scan_inputs {
    const double *odom0, *odom1;       /* [B][3], may be NULL when want_flow == 0 */
    const int32_t *det_offsets;        /* [B+1] or NULL */
    const double *det_rphi;            /* [D][2] */
    const uint8_t *det_cls;            /* [D] */
    int32_t B, D, flow_kind, want_flow;
    double assoc_radius[3];
    int32_t labels[3];
    int32_t pad_;
    double dyn_radius[3];
    void *workspace;
    size_t workspace_bytes;
} pof_scan_inputs;

int pof_scan_preprocess_chained(const float *ranges, long long sample_stride, int B, int N,
                                const double *tab, const double *odom0, const double *odom1,
                                int flow_kind, int canonical, int out_f64, void *xy, void *flow,
                                const int32_t *det_offsets, const double *det_rphi, const uint8_t *det_cls,
                                int D, const double *assoc_radius, const int32_t *labels,
                                const double *dyn_radius, int64_t *closest, int64_t *target_cls,
                                float *target_reg, float *dyn_mask, float *valid_mask, float *exclude_mask,
                                void *workspace, size_t workspace_bytes, const pof_scan_inputs *next,
                                pof_stream_t stream);

/* Several batches per launch (round 3).  A data loader that runs ahead hands over up to
 * POF_SCAN_MAX_SLOTS ring slots at once: ONE launch streams the n_cur batches `cur` (their workspaces must hold
 * their params) and evaluates the params of the n_next batches `next` on extra workgroups, as the chained form
 * does for one.  All batches of a call share N, the angle table, flow_kind / canonical / out_f64, the class
 * constants and the SET of non-NULL outputs (POF_E_BADARG otherwise); B may differ.  n_cur == 0: params only.
 * tab_cs_f32: optional [N][2] float32 copy of the table's (cos, sin) pairs, each rounded once from the float64
 * entry (what the float32-output kernel would otherwise convert per point); NULL is allowed.
 * Shapes: N even, N >= 128 (POF_E_SHAPE otherwise: use pof_scan_preprocess_chained), sample_stride even.
 * Alignment: ranges 8-byte and every non-NULL output 16-byte aligned; there is no fallback: POF_E_SHAPE otherwise
 * (use pof_scan_preprocess_chained for such buffers).
 * Replaces the same reference calls as pof_scan_preprocess (dataset_dr_spaam.py:384-409), for a window of
 * consecutive DataLoader batches (dataset_dr_spaam.py:26-28, prefetching workers). */
#define POF_SCAN_MAX_SLOTS 8
typedef struct pof_scan_batch {
    const float *ranges;               /* row b at ranges + b * sample_stride */
    long long sample_stride;
    int32_t B, D;
    const int32_t *det_offsets;        /* [B+1] or NULL */
    void *xy, *flow;                   /* [B][N][2] float32 / float64 (out_f64), or NULL */
    int64_t *closest, *target_cls;     /* [B][N] or NULL */
    float *target_reg;                 /* [B][N][2] or NULL */
    float *dyn_mask, *valid_mask, *exclude_mask;   /* [B][N] or NULL */
    void *workspace;
    size_t workspace_bytes;
} pof_scan_batch;

int pof_scan_preprocess_multi(const pof_scan_batch *cur, int n_cur, const pof_scan_inputs *next, int n_next,
                              int N, const double *tab, const float *tab_cs_f32, int flow_kind, int canonical,
                              int out_f64, const double *assoc_radius, const int32_t *labels,
                              const double *dyn_radius, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A3 on caller-supplied scanner-frame points (the reference's own signature):
 *   get_displacement_from_odometry(scan1_xy, odom0, odom1)   src/utils/utils.py:639-662
 *   get_velocity_from_odometry(scan1_xy, odom0, odom1)       src/utils/utils.py:609-636
 * xy, flow [B][N][2] float64; odom [B][3]; tab only needed when canonical != 0.
 * ---------------------------------------------------------------------- */
int pof_flow_from_xy(const double *xy, const double *odom0, const double *odom1, int flow_kind,
                     int canonical, const double *tab, double *flow, int B, int N,
                     pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A2 inverse  xy_to_rphi(x, y) -> (hypot, atan2(y, x))   src/utils/utils.py:39-43
 * float64, n elements.
 * ---------------------------------------------------------------------- */
int pof_xy_to_rphi(const double *x, const double *y, double *r, double *phi, long long n,
                   pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A4 stand-alone frame rotation of a flow field
 *   global_to_canonical_flow / canonical_to_global_flow(_torch)
 *                                             src/utils/utils.py:62-105
 * flow_in/out [B][N][2], float32 (is_f64=0) or float64; may alias.
 * ---------------------------------------------------------------------- */
int pof_rotate_flow(const void *flow_in, void *flow_out, const double *tab, int B, int N,
                    int to_canonical, int is_f64, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A5 global_to_canonical / canonical_to_global   src/utils/utils.py:55-59,109-126
 * Batched over [B][N]; det_* and d* are per point.  float64.
 * ---------------------------------------------------------------------- */
int pof_det_to_canonical(const float *ranges, const double *tab, const double *det_r,
                         const double *det_phi, double *dx, double *dy, int B, int N,
                         pof_stream_t stream);
int pof_canonical_to_det(const float *ranges, const double *tab, const double *dx, const double *dy,
                         double *det_r, double *det_phi, int B, int N, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A8 scans_to_cutout                            src/utils/utils.py:259-334
 * scans [B][T][N] float32 -> out [B][N/stride][T][P] float32.
 * workspace: int32[B] (per-sample area factor), caller provided.
 * half-angle arctangent: correctly rounded float32.
 * dbg_lo (optional, may be NULL): [B][P][T][N/stride] int32 copy of
 * inds_ct_low for the bit-exact index tests.
 * ---------------------------------------------------------------------- */
int pof_cutout(const float *scans, int B, int T, int N, const double *tab, int stride, int centered,
               int fixed, double window_width, double window_depth, int num_cutout_pts,
               double padding_val, int area_mode, float *out, int32_t *workspace,
               int32_t *dbg_lo, pof_stream_t stream);

/* Same with a value-path selector: value_mode 0 = float64 value path (bit-exact, what
 * pof_cutout runs); 1 = float32 value path: the index math stays float64 and exact
 * (same inds_ct_low / out-of-range / area indices), only lerp, clip and centring run in
 * float32 (|error| <= 1e-5 in the normalised output).  Compare: the reference's own
 * scans_to_cutout_torch does its INDEX math in float32 (src/utils/utils.py:337-420). */
int pof_cutout_ex(const float *scans, int B, int T, int N, const double *tab, int stride, int centered,
                  int fixed, double window_width, double window_depth, int num_cutout_pts,
                  double padding_val, int area_mode, int value_mode, float *out, int32_t *workspace,
                  int32_t *dbg_lo, pof_stream_t stream);

/* BASELINE config 5 storage (reference src/utils/utils.py:259-334 returns float32): the same cutout
 * written as IEEE float16 (the float32 result
 * rounded to nearest even once more), out_f16 [B][ceil(N/stride)][T][P] half.  Halves the
 * dominant write traffic (3600*11*(4 + 56*2) bytes per dense sample).
 * Alignment (this call, pof_cutout and pof_cutout_ex): none required.  Rows are staged in LDS with float2 loads
 * only when scans is 8-byte aligned and T*N even (scalar loads otherwise); outputs are written as float4 / half4
 * only when P % 4 == 0 and out is 16-byte aligned (scalar stores otherwise).  The bits do not depend on either. */
int pof_cutout_f16(const float *scans, int B, int T, int N, const double *tab, int stride, int centered,
                   int fixed, double window_width, double window_depth, int num_cutout_pts,
                   double padding_val, int area_mode, int value_mode, void *out_f16, int32_t *workspace,
                   int32_t *dbg_lo, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A11 nms_predicted_center                      src/utils/utils.py:535-571
 * One scan per batch entry.  pred_cls [B][N] float64 scores, pred_reg [B][N][2].
 * Outputs: det_xy [B][N][2] float64 and det_cls [B][N] float64 compacted to the
 * first num_det[b] rows, instance_mask [B][N] int32.  Scores must be distinct
 * (the reference's argsort is unstable on ties).
 * workspace: at least pof_nms_workspace_bytes(B, N) bytes.
 * ---------------------------------------------------------------------- */
size_t pof_nms_workspace_bytes(int B, int N);
int pof_nms_predicted_center(const float *ranges, const double *tab, const double *pred_cls,
                             const double *pred_reg, double min_dist, int B, int N, double *det_xy,
                             double *det_cls, int32_t *num_det, int32_t *instance_mask,
                             void *workspace, size_t workspace_bytes, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N5 per-person flow in the world frame
 *   depracted_scripts/infer_person_flow.py:134-157, src/utils/viz_utils.py:556-575 (plot_person_flow_fixed_pose)
 * One scan per batch entry, one launch.  Inputs: flow_canonical [B][N][2] float32 (a flow net's output), the
 * NMS results instance_mask [B][N], num_det [B], det_xy [B][N][2], det_cls [B][N], and per scan the sensor pose
 * as the reference holds it: rot [B][4] = _phi_to_rotation_matrix(odom1[2]) (src/utils/utils.py:601-606, float32,
 * row-major), trans [B][2] = odom1[:2], flow_trans [B][2] = (odom1 - odom0)[:2].
 * Per point:  flow_global [B][N][2] float32 = canonical_to_global_flow_torch (utils.py:92-105; the bits of
 *   pof_rotate_flow);  flow_world [B][N][2] float64 = np.matmul(flow_global, rot.T) + flow_trans, the product in
 *   float32 as fmaf(g1, Rt[1][c], g0 * Rt[0][c]);  rgb [B][N][3] float64 = flow_to_hsv(flow_world) (utils.py:574-584).
 * Per detection k < num_det[b] (instance id k + 1; ids outside [1, num_det[b]] are ignored, num_det is clamped to
 *   [0, N]):  det_count [B][N] int32 = its points;  det_flow [B][N][2], det_rgb [B][N][3] = np.mean of flow_world /
 *   rgb over them, summed in ascending point index with float64 adds (deterministic; count 0 -> NaN);
 *   det_xy_world [B][N][2] = fma(d1, Rt[1][c], d0 * Rt[0][c]) + trans (np.matmul(dets_xy, rot.T) + odom1[:2]);
 *   det_valid [B][N] uint8 = det_cls >= cls_thresh (the reference draws dets_cls[j] < cls_thresh black).
 *   Rows k >= num_det[b] of the five per-detection outputs are written as zeros.
 * N <= 4096 (POF_E_SHAPE beyond, as for the NMS); one wave per scan up to N = 512.
 * ---------------------------------------------------------------------- */
int pof_person_flow(const float *flow_canonical, const double *tab, const int32_t *instance_mask,
                    const int32_t *num_det, const double *det_xy, const double *det_cls, const float *rot,
                    const double *trans, const double *flow_trans, double cls_thresh, int B, int N,
                    float *flow_global, double *flow_world, double *rgb, double *det_xy_world, double *det_flow,
                    double *det_rgb, int32_t *det_count, uint8_t *det_valid, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N6 ego-motion from a flow field: the weighted least-squares inverse of
 *   get_displacement_from_odometry(scan1_xy, odom0, odom1)   src/utils/utils.py:639-662
 *   get_velocity_from_odometry(scan1_xy, odom0, odom1)       src/utils/utils.py:609-636
 * One scan per batch entry, one launch.  Points p: xy [B][N][2] float64, or, when xy is NULL, ranges [B][N] float32
 * placed by tab as rphi_to_xy does (r * cos, r * sin).  flow [B][N][2] float32 (flow_f64 = 0) or float64; with
 * canonical != 0 it is first rotated to the scanner frame in its own type (the bits of pof_rotate_flow).  g = sign * f
 * (sign = +-1; -1 for the reference's displacement, disp = p_now - p_prev), q = p + g.
 * Base weight w0 = weight [B][N] float32 (NULL: 1), forced to 0 when the weight is not finite or <= 0, when ranges is
 * given and r is not finite or >= max_range (the reference's valid mask is r < 20), when a flow or point component is
 * not finite, and -- with instance_mask [B][N] -- when 1 <= id <= clamp(num_det[b], 0, N) and
 * det_cls[b][id - 1] >= cls_thresh (pof_person_flow's det_valid: the point belongs to a person).
 * model 0 (rigid, any angle): theta = atan2(S_x, S_dot), u = qm - R(theta) pm over the centred weighted moments;
 * model 1 (linear twist g = t + omega * (-y, x)): omega = sum w (p'_x g'_y - p'_y g'_x) / S_pp, t = gm - omega (-pm_y, pm_x).
 * A solve fails with fewer than two points of weight > 0 or S_pp not > 0.  huber_delta > 0 re-weights `iters` (0..16)
 * times, w = w0 * (rho > delta ? delta / rho : 1) with rho the point's residual length.
 * Outputs: motion [B][3] float64 = (theta, u_x, u_y) or (omega, t_x, t_y), NaN when a solve failed; count [B] int32 =
 *   points with w0 > 0; rms [B] = sqrt(sum w rho^2 / W) of the last solve; ok [B] uint8; optional flow_residual
 *   [B][N][2] float64 = the flow minus the fitted motion's flow at every point (scanner frame); optional weight_out
 *   [B][N] float32 = the last solve's weights.
 * Sums have a fixed order (no atomics): the same bits in every run, at every batch position, in a graph replay.
 * N <= 4096 (POF_E_SHAPE beyond, as for the NMS); one wave per scan up to N = 512.
 *
 * pof_pose_advance composes a rigid motion (displacement convention) onto pose [B][3] = (x, y, phi), in place:
 *   ok:  phi1 = phi0 + theta, t1 = t0 + R(phi0) u;  otherwise the pose stays.  It also writes (each may be NULL) what
 *   pof_person_flow reads: rot [B][4] float32 of (cos phi1, -sin phi1, sin phi1, cos phi1), trans [B][2] = t1,
 *   flow_trans [B][2] = t1 - t0 (zeros without ok).
 * ---------------------------------------------------------------------- */
int pof_ego_motion(const float *ranges, const double *xy, const double *tab, const void *flow, int flow_f64,
                   int canonical, int sign, int model, const float *weight, const int32_t *instance_mask,
                   const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range,
                   double huber_delta, int iters, int B, int N, double *motion, int32_t *count, double *rms,
                   uint8_t *ok, double *flow_residual, float *weight_out, pof_stream_t stream);
int pof_pose_advance(const double *motion, const uint8_t *ok, double *pose /* [B][3] in/out */, float *rot,
                     double *trans, double *flow_trans, int B, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N7 person tracks: gated greedy nearest-neighbour association of a scan's detections with persistent tracks, and a
 * constant-velocity Kalman filter per track whose time step is one scan.  The reference has no tracker; the
 * specification is this comment (restated in float64 NumPy by tests/test_tracks.py).
 * One sensor per batch entry, one launch.  Inputs, as pof_person_flow and the NMS write them: det_xy_world [B][N][2],
 * det_flow [B][N][2] float64, det_valid [B][N] uint8, num_det [B] (clamped to [0, N]), instance_mask [B][N].
 * State, in place, M = max_tracks slots per sensor: track_id [B][M] int32 (0 = free), track_state [B][M][4] float64 =
 * (x, y, vx, vy) with the velocity in metres per scan, track_cov [B][M][3] float64 = (a, b, c) = position variance,
 * position/velocity covariance, velocity variance (one 2x2 block for both axes: every noise is isotropic),
 * track_hits / track_misses / track_age [B][M] int32, next_id [B] int32 (starts at 1).
 * One step, float64, plain multiplies and adds in this order (no FMA):
 *   1. every live slot:  x += vx, y += vy;  a <- (a + b) + (b + c), b <- b + c, c <- c + q;  age += 1
 *   2. candidates: rows k < num_det with det_valid[k] != 0 and both centre components finite
 *   3. cost(t, k) = dx dx + dy dy, dx = zx - x, dy = zy - y; a pair takes part while cost <= gate gate
 *   4. repeatedly the pair of smallest cost among unassigned slots and candidates; ties go to the lower slot, then the
 *      lower row; stop when no pair is inside the gate
 *   5. matched slot:  s = a + r_pos, k1 = a / s, k2 = b / s, r = z - p;  p += k1 r, v += k2 r;
 *        (a, b, c) <- (a - k1 a, b - k1 b, c - k2 b);
 *      then, if both components of the row's det_flow f are finite:  s = c + r_vel, k1 = b / s, k2 = c / s, r = f - v;
 *        p += k1 r, v += k2 r;  (a, b, c) <- (a - k1 b, b - k1 c, c - k2 c);
 *      hits += 1, misses = 0
 *   6. unmatched live slot: misses += 1; beyond max_misses the slot is freed and all its fields are zeroed
 *   7. births: unmatched candidates in ascending row order, each into the lowest free slot (slots freed in 6 count):
 *      id = next_id++, p = z, v = f if finite else 0, cov = (r_pos, 0, r_vel) if f was finite else (r_pos, 0, v0_var),
 *      hits = 1, misses = 0, age = 0; with no free slot dropped += 1
 * Outputs, overwritten every step: track_det [B][M] int32 = the detection row the slot was matched with or born from
 *   in this step, else -1; track_confirmed [B][M] uint8 = live and hits >= min_hits; det_track [B][N] int32 = the
 *   track id of each detection row or 0; point_track [B][N] int32 = det_track[instance - 1], 0 for instance ids
 *   outside [1, num_det]; dropped [B] int32 = candidates that found no free slot in this step.
 * One wave per sensor, no atomics: the same bits in every run, at every batch position and in a graph replay.
 * max_tracks <= 256, N <= 4096 (POF_E_SHAPE beyond, nothing touched); every row may be a candidate (the candidate cap
 * is N).  gate, q >= 0 and r_pos, r_vel, v0_var > 0, max_misses >= 0 (POF_E_BADARG otherwise).
 * ---------------------------------------------------------------------- */
int pof_track_update(const double *det_xy_world, const double *det_flow, const uint8_t *det_valid,
                     const int32_t *num_det, const int32_t *instance_mask, int B, int N, int max_tracks,
                     int32_t *track_id, double *track_state, double *track_cov, int32_t *track_hits,
                     int32_t *track_misses, int32_t *track_age, int32_t *next_id, int32_t *track_det,
                     uint8_t *track_confirmed, int32_t *det_track, int32_t *point_track, int32_t *dropped,
                     double gate, double q, double r_pos, double r_vel, double v0_var, int max_misses, int min_hits,
                     pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N8 scan-to-scan matching: the sensor's motion between two consecutive scans without a flow field, a point-to-line
 * ICP of the current scan against the previous one.  On a static scene it inverts
 *   get_displacement_from_odometry(scan1_xy, odom0, odom1)   src/utils/utils.py:639-662
 * and has the (theta, u) convention of pof_ego_motion's rigid model (sign = -1): a point now at p was at
 * R(theta) p + u; pof_pose_advance takes the result unchanged.  The reference has no scan matcher; the specification
 * is this comment (restated in float64 NumPy by tests/test_scan_match.py).
 * One scan pair per batch entry, one launch.  ranges_prev, ranges_cur [B][N] float32; tab the angle table.
 * Points: a_j = r_prev[j] * (cos, sin)[j], p_i = r_cur[i] * (cos, sin)[i] in float64, as rphi_to_xy.  A range is
 * valid when finite and < max_range.  A current point is also left out when -- with instance_mask [B][N] -- 1 <= id <=
 * clamp(num_det[b], 0, N) and det_cls[b][id - 1] >= cls_thresh (as pof_ego_motion: people do not vote).
 * dphi = tab[1] - tab[0] (0 for N = 1).  Start (theta, u) = init [B][3] float64, zeros when init is NULL or a
 * component of the row is not finite.  init may be the motion buffer (a row is read before it is written).
 * Correspondence of p_i at (theta, u), (c, s) = (cos theta, sin theta):
 *   shift = (int)clamp(rint(theta / dphi), -N, N)  (0 when dphi == 0; a NaN quotient gives -N)
 *   q = ((c p_x - s p_y) + u_x, (s p_x + c p_y) + u_y)
 *   j = the valid vertex of smallest d2 = (q_x - a_jx)^2 + (q_y - a_jy)^2 over [i + shift - window, i + shift + window]
 *       clamped to [0, N), ties to the lower j; unmatched without one or when not d2 <= gate^2.
 *   k in {j - 1, j + 1}: inside [0, N), valid, e = a_k - a_j with 0 < |e|^2 <= max_gap^2; of two the one with the
 *       smaller |q - a_k|^2, j - 1 on a tie; unmatched without one.
 *   len = sqrt(|e|^2), n = (-e_y / len, e_x / len), d = q - a_j, r = n_x d_x + n_y d_y.
 * One iteration: w = |r| > huber_delta ? huber_delta / |r| : 1 (1 when huber_delta == 0),
 *   J = (n_x (-q_y) + n_y q_x, n_x, n_y); over the matched points A = sum w J J^T (terms w (J_a J_b)),
 *   g = sum w (J r), sum w, sum w (r r), and their number.  The pair fails with fewer than 3 matched points (obs = 0).
 *   dmax = max(A00, A11, A22); Cholesky with every pivot tested as it is formed, the pair fails at the first pivot that
 *   is not > min_pivot * dmax (a corridor: the translation along it is not observable):
 *     p0 = A00, l00 = sqrt(p0), l10 = A01 / l00, l20 = A02 / l00
 *     p1 = A11 - l10 l10, l11 = sqrt(p1), l21 = (A12 - l20 l10) / l11
 *     p2 = (A22 - l20 l20) - l21 l21, l22 = sqrt(p2);   obs = min(pivots formed) / dmax (0 when dmax is not > 0)
 *     y0 = -g0 / l00, y1 = (-g1 - l10 y0) / l11, y2 = ((-g2 - l20 y0) - l21 y1) / l22
 *     x2 = y2 / l22, x1 = (y1 - l21 x2) / l11, x0 = ((y0 - l10 x1) - l20 x2) / l00
 *   (c0, s0) = (cos x0, sin x0): theta += x0, u <- ((c0 u_x - s0 u_y) + x1, (s0 u_x + c0 u_y) + x2).
 *   Stop after `iters` (1..32) iterations or when |x0| < eps_theta and max(|x1|, |x2|) < eps_u.
 * Outputs: motion [B][3] float64 = (theta, u_x, u_y), NaN when the pair failed; count [B] int32 = points matched in
 *   the last iteration; rms [B] = sqrt(sum w r r / sum w) of the last iteration (NaN when failed); ok [B] uint8;
 *   iters_used [B] int32; obs [B] float64 of the last solve.  After the last iteration one more correspondence pass at
 *   the final (theta, u) writes (each may be NULL) corr [B][N] int32 = j or -1 and flow_residual [B][N][2] float64 =
 *   (c d_x + s d_y, -s d_x + c d_y), the nearest-vertex displacement turned back into the current scanner frame, NaN
 *   where unmatched (all -1 / NaN for a failed pair).
 * Sums have a fixed order (no atomics, no FMA): the same bits in every run, at every batch position, in a graph
 * replay.  N <= 4096 (POF_E_SHAPE beyond, nothing written); one wave per pair up to N = 512.  POF_E_BADARG: window
 * outside 1..64, iters outside 1..32, gate, max_gap or huber_delta not >= 0.
 * ---------------------------------------------------------------------- */
int pof_scan_match(const float *ranges_prev, const float *ranges_cur, const double *tab, const double *init,
                   const int32_t *instance_mask, const int32_t *num_det, const double *det_cls, double cls_thresh,
                   double max_range, int window, double gate, double max_gap, double huber_delta, int iters,
                   double eps_theta, double eps_u, double min_pivot, int B, int N, double *motion, int32_t *count,
                   double *rms, uint8_t *ok, int32_t *iters_used, double *obs, int32_t *corr, double *flow_residual,
                   pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N9 keyframe scan matching: the current scan is matched against a reference scan (the keyframe) that stays fixed
 * until the sensor has moved away from it; the pose is key_pose o (theta, u), so no fit error accumulates while one
 * keyframe is held.  The reference has no scan matcher; the specification is this comment together with N8's
 * (restated in float64 NumPy by tests/test_keyframe.py).  One sensor per batch entry, one launch.
 * State per sensor, persistent, updated in place, allocated by the caller:
 *   key_ranges [B][N] float32 (NaN = not a vertex), key_pose [B][3] float64 = (x, y, phi) of the keyframe,
 *   key_rel [B][3] float64 = (theta, u) of the last good match against it, key_valid [B] uint8, key_age [B] int32 =
 *   scans since the keyframe was taken, key_misses [B] int32 = failed matches in a row, pose [B][3] float64.
 * Convention as N8: a point now at p was at R(theta) p + u in the keyframe's scanner frame, and the composition is
 *   pof_pose_advance's: key_pose o (theta, u) = (t_k + R(phi_k) u, phi_k + theta) with
 *   x = x_k + (c u_x - s u_y), y = y_k + (s u_x + c u_y), (c, s) = (cos phi_k, sin phi_k).
 * Points: vertices a_j = key_ranges[j] * (cos, sin)[j], valid when the range is finite and < max_range (a stored NaN
 *   is not); current points p_i, their validity and the NMS gate (instance_mask, num_det, det_cls, cls_thresh) exactly
 *   as N8.  A current point that is valid and not gated `votes`; V = their number.  The gated current scan is the row
 *   g[i] = votes ? ranges_cur[i] : NaN -- people standing in a scan that becomes the keyframe are never vertices.
 * Correspondence of p at (theta, u): q as N8, then
 *   mid = (int)clamp(rint((atan2(q_y, q_x) - tab[0]) / dphi), -N, 2N)   (0 when dphi == 0; a NaN gives -N)
 *   j = the valid vertex of smallest d2 over [mid - window, mid + window] n [0, N), scanned upwards with a strict <.
 *   No wrap-around: a point that projects more than `window` beams outside the keyframe's field of view is unmatched.
 *   Everything after that -- the gate, the line partner, n, d, r, w, J, the twelve sums, the Cholesky with its pivot
 *   tests, obs, the composition and the stop rule -- is N8's, operation for operation.
 * One step of a sensor (old = the pose on entry):
 *   1. key_valid == 0 (seeding): key_ranges <- g, key_pose = old, key_rel = 0, key_age = 0, key_misses = 0,
 *      key_valid = 1; ok = 0, motion and rms NaN, count = 0, iters_used = 0, obs = 0, key_replaced = 1, corr -1,
 *      flow_residual NaN; the pose stays.
 *   2. otherwise the match runs from key_rel (zeros when a component is not finite) and key_age counts this scan.
 *   3. match ok: key_rel = (theta, u), pose = key_pose o key_rel, key_misses = 0.  The keyframe is replaced when
 *      |theta| > key_rot  or  u_x u_x + u_y u_y > key_dist key_dist  or  (double)count < min_share * V:
 *      key_ranges <- g, key_pose = pose, key_rel = 0, key_age = 0; otherwise key_age += 1.
 *   4. match failed: the pose and key_rel stay, motion NaN.  key_misses + 1 > max_misses re-anchors: key_ranges <- g,
 *      key_pose = old, key_rel = 0, key_age = 0, key_misses = 0; otherwise key_misses += 1 and key_age += 1.
 * Outputs: motion [B][3] = the (theta, u) the pose was formed from (NaN without ok); count, rms, ok, iters_used, obs
 *   as N8; key_replaced [B] uint8; optional corr [B][N] and flow_residual [B][N][2] as N8, against the keyframe that
 *   was matched (before any replacement); optional, as pof_pose_advance writes them for pof_person_flow, rot [B][4]
 *   float32 of the new phi, trans [B][2] = the new t, flow_trans [B][2] = t_new - t_old (zeros without ok).
 * A workgroup reads its key_ranges row only while staging and writes it after the last correspondence pass, every
 * thread the beams it staged: the replacement needs no second buffer.  Fixed summation order, no atomics, no FMA: the
 * same bits in every run, at every batch position, in a graph replay.  N <= 4096 (POF_E_SHAPE beyond, nothing
 * written); one wave per sensor up to N = 512.  POF_E_BADARG: as N8, and key_dist, key_rot or min_share not >= 0,
 * max_misses < 0.
 * ---------------------------------------------------------------------- */
int pof_keyframe_match(const float *ranges_cur, const double *tab, const int32_t *instance_mask,
                       const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range, int window,
                       double gate, double max_gap, double huber_delta, int iters, double eps_theta, double eps_u,
                       double min_pivot, double key_dist, double key_rot, double min_share, int max_misses, int B,
                       int N, float *key_ranges, double *key_pose, double *key_rel, uint8_t *key_valid,
                       int32_t *key_age, int32_t *key_misses, double *pose, double *motion, int32_t *count,
                       double *rms, uint8_t *ok, int32_t *iters_used, double *obs, uint8_t *key_replaced,
                       int32_t *corr, double *flow_residual, float *rot, double *trans, double *flow_trans,
                       pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N10 keyframe map: N9 with a ring of `keys` = K keyframes per sensor.  The scan is matched against the ACTIVE keyframe
 * exactly as N9 matches against its only one; when the sensor leaves it, it first looks for a stored keyframe it has
 * come back to and switches to that one instead of storing a new one.  The next match against a revisited keyframe k
 * gives pose = key_pose[k] o match: everything accumulated since k was stored is dropped, so the drift is bounded by
 * the area the ring covers and not by the distance travelled.  The reference has no scan matcher; the specification is
 * this comment together with N8's and N9's (restated in float64 NumPy by tests/test_keyframe_map.py).  One sensor per
 * batch entry, one launch.
 * State per sensor, persistent, updated in place, allocated by the caller:
 *   key_ranges [B][K][N] float32 (NaN = not a vertex), key_pose [B][K][3] float64 = (x, y, phi) of every stored
 *   keyframe, key_valid [B][K] uint8 = the slot holds a keyframe, key_stamp [B][K] int32 = the value of `step` when the
 *   slot was last active, key_active [B] int32 = the active slot (a value outside [0, K) is read as the nearest slot),
 *   key_rel [B][3] float64 = (theta, u) of the last good match against the active slot, key_age [B] int32 = scans on
 *   the active slot, key_misses [B] int32 = failed matches in a row, step [B] int32 = the scan counter, pose [B][3]
 *   float64.
 * Settings: N9's, keys (1..64) and revisit in [0, 1].  Points, the gated current scan g, V, the correspondence with
 * its beam-projected window centre, the iterations and the composition key_pose o (theta, u): N9's, operation for
 * operation.
 * One step of a sensor (a = key_active, old = the pose on entry):
 *   1. key_valid[a] == 0 (seeding): N9's rule 1 on slot a -- key_ranges[a] <- g, key_pose[a] = old, key_valid[a] = 1,
 *      key_rel = 0, key_age = 0, key_misses = 0; ok = 0, motion and rms NaN, count = 0, iters_used = 0, obs = 0,
 *      key_replaced = 1, corr -1, flow_residual NaN; the pose stays.
 *   2. otherwise the match runs against slot a from key_rel (zeros when a component is not finite), exactly N9's;
 *      corr and flow_residual are written against slot a.
 *   3. match ok: key_rel = (theta, u), pose = key_pose[a] o key_rel, key_misses = 0.  With
 *        left  = |theta| > key_rot  or  u_x u_x + u_y u_y > key_dist key_dist
 *        stale = (double)count < min_share * V
 *      neither: the keyframe is held, key_age += 1.
 *      left (whether or not stale): for every valid slot k != a, in ascending k, the pose relative to that keyframe
 *          theta_k = remainder(phi - phi_k, 2 pi)  (the IEEE remainder),  d = t - t_k,  (c_k, s_k) = (cos, sin) phi_k,
 *          u_k = (c_k d_x + s_k d_y, (-s_k) d_x + c_k d_y),  d2_k = u_kx u_kx + u_ky u_ky;
 *        k qualifies when |theta_k| <= revisit * key_rot and d2_k <= (revisit * key_dist) (revisit * key_dist); the
 *        winner is the qualifying slot of smallest d2_k, compared with a strict <: ties go to the lower k.
 *        With a winner the sensor SWITCHES: key_active = k, key_rel = (theta_k, u_k), key_age = 0, key_switched = 1;
 *          nothing is stored and the pose stays the one just formed from slot a -- the next scan's match against k
 *          re-anchors it.
 *        Without one a NEW KEYFRAME is stored: slot = the lowest k with key_valid == 0; if there is none the valid slot
 *          k != a of smallest key_stamp (strict <: the lower k on a tie); if there is none either (K = 1) a.  Then
 *          key_ranges[slot] <- g, key_pose[slot] = pose, key_valid[slot] = 1, key_active = slot, key_rel = 0,
 *          key_age = 0, key_replaced = 1.
 *      stale only: the sensor has not left, the place has changed -- slot a is overwritten in place as N9's rule 3:
 *        key_ranges[a] <- g, key_pose[a] = pose, key_rel = 0, key_age = 0, key_replaced = 1.
 *   4. match failed: N9's rule 4 on slot a; re-anchoring overwrites slot a at the unchanged pose.
 *   5. always: key_stamp[key_active] = step for the slot that is active at the end, then step += 1.
 * Outputs: N9's (motion, count, rms, ok, iters_used, obs, key_replaced; optional corr, flow_residual, rot, trans,
 *   flow_trans) and key_switched [B] uint8, key_slot [B] int32 = the active slot at the end.
 * Properties:
 *   With K = 1 every field and output has the bits of pof_keyframe_match on the same scans.
 *   A workgroup reads and writes only its own sensor's rows.  The row of the active slot is read before the first
 *   barrier; any row is written after the last correspondence pass, every thread the beams it staged: N9's in-place
 *   argument, and a write to another slot has no hazard at all.  The slot search runs in every thread over the same
 *   values in ascending k -- the same decision everywhere, no atomics -- and the scalar state is written only after a
 *   barrier behind it.  Fixed summation order, no FMA: the same bits in every run, at every batch position, in a graph
 *   replay.  N <= 4096 (POF_E_SHAPE beyond, nothing written); one wave per sensor up to N = 512.  POF_E_BADARG: as N9,
 *   keys outside 1..64, revisit outside [0, 1] (or NaN), a NULL state or required output pointer.
 * ---------------------------------------------------------------------- */
int pof_keyframe_map_match(const float *ranges_cur, const double *tab, const int32_t *instance_mask,
                           const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range,
                           int window, double gate, double max_gap, double huber_delta, int iters, double eps_theta,
                           double eps_u, double min_pivot, double key_dist, double key_rot, double min_share,
                           int max_misses, double revisit, int B, int N, int keys, float *key_ranges, double *key_pose,
                           uint8_t *key_valid, int32_t *key_stamp, int32_t *key_active, double *key_rel,
                           int32_t *key_age, int32_t *key_misses, int32_t *step, double *pose, double *motion,
                           int32_t *count, double *rms, uint8_t *ok, int32_t *iters_used, double *obs,
                           uint8_t *key_replaced, uint8_t *key_switched, int32_t *key_slot, int32_t *corr,
                           double *flow_residual, float *rot, double *trans, double *flow_trans, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N11 person motion without a flow net: per detection the centroid of its own scan points in the world frame, paired
 * with a centroid of the previous scan by a strict mutual-nearest rule; the difference is the person's displacement
 * per scan.  It has the shape and meaning of pof_person_flow's det_flow, so pof_track_update takes det_xy_world /
 * det_flow / det_valid unchanged.  The reference has nothing of the kind; the specification is this comment (restated
 * in float64 NumPy by tests/test_person_motion.py).  One sensor per batch entry, one launch.
 * Inputs: ranges [B][N] float32, the current scan; tab the angle table; the NMS results instance_mask [B][N], num_det
 *   [B] (clamped to [0, N]), det_xy [B][N][2], det_cls [B][N]; the pose terms as pof_pose_advance and the keyframe
 *   launches write them, rot [B][4] float32 row-major = (R00, R01, R10, R11) and trans [B][2] = (t_x, t_y).
 * State per sensor, persistent, updated in place, allocated by the caller: prev_centre [B][N][2] float64, prev_cand
 *   [B][N] uint8, prev_num [B] int32 (clamped to [0, N] when read).  A reset state has prev_num = 0: the launch runs
 *   from the first scan of a sequence on and seeds itself there.
 * Per detection row k < num_det:
 *   det_xy_world [B][N][2] = fma(d1, Rt[1][c], d0 * Rt[0][c]) + trans and det_valid [B][N] uint8 = det_cls >= cls_thresh:
 *     pof_person_flow's expressions, and its bits for the same inputs.
 *   A point i counts for row k when instance_mask[i] = k + 1 and ranges[i] is finite and < max_range.  Its world
 *     position, float64, plain multiplies and adds (no FMA):  r = (double)ranges[i], p = (r cos_i, r sin_i),
 *     w_x = ((double)R00 p_x + (double)R01 p_y) + t_x,  w_y = ((double)R10 p_x + (double)R11 p_y) + t_y.
 *   det_count [B][N] int32 = the number of counted points; det_centre [B][N][2] = the sum of their w, added in
 *     ascending point index with float64 adds starting from 0, divided by (double)det_count (count 0 -> NaN).
 *   Row k is a candidate when det_valid, det_count >= min_points and both centre components are finite.
 * Association with the previous scan's candidate rows (j < prev_num with prev_cand[j] != 0):
 *   d2(k, j) = dx dx + dy dy with d = det_centre[k] - prev_centre[j]; it counts only while d2 <= reach reach.
 *   best(k) of a current candidate k: the previous candidate j of smallest d2, j scanned upwards with a strict <.
 *   back(j) of a previous candidate j: the current candidate k of smallest d2, k scanned upwards with a strict <
 *     (the lower k keeps a tie).
 *   (k, j) is a pair when j = best(k) and k = back(j).  Then det_flow [B][N][2] = det_centre[k] - prev_centre[j] and
 *   det_prev [B][N] int32 = j; otherwise det_flow is NaN and det_prev -1 (pof_track_update then makes its position-only
 *   update by itself).
 * Rows k >= num_det of the six outputs are zeros, with det_prev = -1.
 * State update, after every read of it: prev_centre = det_centre, prev_cand = the candidate flags (0 from num_det on),
 *   prev_num = the clamped num_det.
 * One workgroup per sensor that reads and writes only its own rows; no atomics, fixed order: the same bits in every
 * run, at every batch position and in a graph replay.  N <= 4096 (POF_E_SHAPE beyond, nothing written); one wave per
 * sensor up to N = 512.  POF_E_BADARG: a NULL pointer, reach not >= 0, min_points < 1, B < 0, N < 1.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_person_motion(const float *ranges, const double *tab, const int32_t *instance_mask, const int32_t *num_det,
                      const double *det_xy, const double *det_cls, const float *rot, const double *trans,
                      double cls_thresh, double max_range, double reach, int min_points, int B, int N,
                      double *prev_centre, uint8_t *prev_cand, int32_t *prev_num, double *det_xy_world,
                      double *det_flow, double *det_centre, int32_t *det_count, uint8_t *det_valid, int32_t *det_prev,
                      pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N12 occupancy grid map: a log-odds grid per sensor, updated by every scan from the scan and the pose terms.  It says
 * which cells were seen free and which occupied, and per scan point what its cell held before this scan: a walking
 * person's points land on cells that were seen free, the points of a static object do not.  The reference has nothing
 * of the kind; the specification is this comment (restated in float64 NumPy by tests/test_grid_map.py).  One sensor
 * per batch entry, two launches on the stream (the points, then the cells).
 * State per sensor, persistent, updated in place, allocated by the caller: grid [B][H][W] int16, the log-odds in integer
 *   counts, 0 = unknown, row iy is y and column ix is x; origin [B][2] float64 = (o_x, o_y), the world position of the
 *   lower corner of cell (0, 0), read only.  A reset state is all zeros.
 * Inputs: ranges [B][N] float32, the current scan; tab the angle table (its cosines and sines lie in [-1, 1], as those
 *   of pof_laser_phi do); the pose terms as pof_pose_advance and the keyframe launches write them, rot [B][4] float32
 *   row-major = (R00, R01, R10, R11) and trans [B][2] = (t_x, t_y): world = R p + t; optionally the NMS results
 *   instance_mask [B][N], num_det [B] (clamped to [0, N]) and det_cls [B][N], all three or none (NULL).
 * Per beam i, float64, plain multiplies and adds (no FMA):  r = (double)ranges[i].  The beam is a HIT when r is finite
 *   and 0 < r < max_range.  p = (r cos_i, r sin_i), w_x = ((double)R00 p_x + (double)R01 p_y) + t_x,
 *   w_y = ((double)R10 p_x + (double)R11 p_y) + t_y (N11's expressions), g_x = floor((w_x - o_x) / res), g_y =
 *   floor((w_y - o_y) / res) with a true division.  The endpoint is INSIDE when 0 <= g_x < W and 0 <= g_y < H, compared
 *   in double (a NaN is outside).  A beam is a PERSON's point when the NMS results are given, id = instance_mask[i]
 *   has 1 <= id <= num_det and det_cls[id - 1] >= cls_thresh (pof_ego_motion's gate): persons are never burned in.
 *     point_cell  [B][N] int32 = g_y W + g_x for a hit inside the grid, else -1;
 *     point_prior [B][N] int16 = the grid value of that cell BEFORE this call's update, -32768 where point_cell is -1;
 *     point_mark  [B][N] uint8 = 1 for a hit inside the grid that is no person's point, else 0.
 * Per detection row k < num_det (NMS results given):  det_points [B][N] int32 = the number of hits inside the grid with
 *   instance_mask = k + 1, det_free [B][N] int32 = how many of them have point_prior <= -free_thresh.  Rows >= num_det,
 *   and every row without NMS results, are zeros.
 * Per cell (ix, iy):  c_x = o_x + ((double)ix + 0.5) res, c_y = o_y + ((double)iy + 0.5) res, d = c - t; in the sensor
 *   frame s_x = (double)R00 d_x + (double)R10 d_y, s_y = (double)R01 d_x + (double)R11 d_y, rho = sqrt(s_x s_x + s_y s_y);
 *   its beam m = rint((atan2(s_y, s_x) - tab[0]) / dphi) with dphi = tab[1] - tab[0] (0 for N = 1), the expression of
 *   the keyframe matcher's window centre; m outside [0, N) (a NaN or an infinity included; no wrap-around) frees nothing.
 *   A beam j is VALID when ranges[j] is not NaN and > 0; then r_eff(j) = min((double)ranges[j], max_range): a beam
 *   without a return frees up to max_range.
 *     1. some beam with point_mark = 1 has this cell as point_cell:                      delta = +hit
 *     2. else beam m is valid and rho + tol < f, f = the smallest r_eff of the valid beams among m - 1, m, m + 1 inside
 *        [0, N) (the neighbours keep a cell beside an occlusion edge from being freed):   delta = -miss
 *     3. else                                                                            delta = 0
 *   grid = (int16)clamp((int)grid + delta, lo, hi) where delta != 0; a cell with delta = 0 keeps its bits.
 * Gather form, no global atomics: the same bits in every run, at every batch position and in a graph replay.
 * POF_E_BADARG (checked first; nothing written): a NULL required pointer, NMS pointers given in part, res not > 0, tol
 *   not >= 0, max_range not > 0, hit < 0, miss < 0, lo outside [-32767, 0], hi outside [0, 32767], free_thresh < 0,
 *   B < 0, N < 1.  POF_E_SHAPE (nothing written): N > 4096, H or W not a multiple of 64 or outside [64, 2048], grid
 *   not 16-byte aligned, B H W / 4096 >= 2^31.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_grid_map_update(const float *ranges, const double *tab, const float *rot, const double *trans,
                        const int32_t *instance_mask, const int32_t *num_det, const double *det_cls, double res,
                        double tol, double max_range, double cls_thresh, int hit, int miss, int lo, int hi,
                        int free_thresh, int B, int N, int H, int W, int16_t *grid, const double *origin,
                        int32_t *point_cell, uint8_t *point_mark, int16_t *point_prior, int32_t *det_points,
                        int32_t *det_free, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N13 scan-to-grid matching: the pose of a sensor corrected against its own occupancy grid (N12).  An exhaustive
 * (correlative) search over whole-cell translations and a small table of rotations around the incoming pose, scored
 * with integers only: it finds a pose that is off by a cell or more (a lost scan pair) to within about a cell and
 * stays silent while the pose is good.  The reference has nothing of the kind; the specification is this comment
 * (restated in NumPy by tests/test_grid_match.py).  One sensor per batch entry, two launches on the stream (the scores,
 * then the pick).
 * Settings: R = reach (0..16), K = rotations (odd, 1..33), T = 2 R + 1; min_points, min_score, min_gain >= 0 (integers;
 *   the last two are grid counts per voting point).
 * Inputs: ranges [B][N] float32, the current scan; tab the angle table; optionally the NMS results instance_mask
 *   [B][N], num_det [B] (clamped to [0, N]) and det_cls [B][N], all three or none (NULL); grid [B][H][W] int16 and
 *   origin [B][2] float64 of N12, both read only; res; rot_tab [K][3] float64 = (theta_k, cos theta_k, sin theta_k),
 *   formed by the host with theta_k = (k - (K - 1) / 2) rot_step, whose middle row is exactly (0, 1, 0) -- the launch
 *   calls no transcendental while it scores.
 * In/out: pose [B][3] float64 = (x, y, phi), and the pose terms as pof_pose_advance writes them, rot [B][4] float32
 *   row-major and trans [B][2] float64.
 * A point i VOTES when r = (double)ranges[i] is finite, 0 < r < max_range, and it is no person's point (N12's rule:
 *   1 <= id <= num_det and det_cls[id - 1] >= cls_thresh).  V = the number of voting points.
 * The cell of a voting point under rotation k, float64, plain multiplies and adds (no FMA), (c, s) = rot_tab[k][1..2]:
 *   p = (r cos_i, r sin_i),  p' = (c p_x - s p_y, s p_x + c p_y),
 *   w_x = ((double)R00 p'_x + (double)R01 p'_y) + t_x,  w_y = ((double)R10 p'_x + (double)R11 p'_y) + t_y with the
 *   INCOMING rot and trans,  g_x = floor((w_x - o_x) / res),  g_y = floor((w_y - o_y) / res) with a true division.
 *   For the middle row p' = p exactly, so g is N12's point_cell arithmetic.
 * scores [B][K][T][T] int32:  scores[b][k][a][e] = the sum over the voting points of grid[g_y + (a - R)][g_x + (e - R)].
 *   A shifted cell outside the grid adds 0 (tested in integers once g is known to be finite); a point whose g_x or g_y
 *   is not finite adds nothing for that k.
 * The pick: best = the largest score; ties go to the smaller dx dx + dy dy (dy = a - R, dx = e - R), then the smaller
 *   |kappa| (kappa = k - (K - 1) / 2), then the smaller flat index (k T + a) T + e.  zero = scores[b][(K - 1) / 2][R][R].
 *   ok    = V >= min_points  and  best >= min_score V
 *   moved = ok  and  the best candidate is not the zero candidate  and  best - zero >= min_gain V
 *   with the products and the difference formed in int64.
 * With moved:  x += (double)dx res,  y += (double)dy res,  phi += theta_k;  pose is written and rot, trans are written
 *   from it as pof_pose_advance writes them.  Without moved pose, rot and trans keep their bits: nothing is stored.
 * Outputs: scores (required: it also carries the sums from the first launch to the second); best [B][3] int32 =
 *   (kappa, dy, dx) of the best candidate, written always; score [B][2] int32 = (best, zero); votes [B] int32 = V;
 *   ok [B], moved [B] uint8; correction [B][3] float64 = ((double)dx res, (double)dy res, theta_k), zeros without moved.
 * Integer sums, no global atomics: the same bits in every run, at every batch position and in a graph replay.
 * POF_E_BADARG (checked first; nothing written): a NULL pointer other than the three NMS results, NMS pointers given
 *   in part, res not > 0, max_range not > 0, reach outside [0, 16], rotations outside [1, 33] or even, min_points,
 *   min_score or min_gain < 0, B < 0, N < 1.  POF_E_SHAPE (nothing written): N > 4096, H or W not a multiple of 64 or
 *   outside [64, 2048].  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_grid_match(const float *ranges, const double *tab, const int32_t *instance_mask, const int32_t *num_det,
                   const double *det_cls, double cls_thresh, double max_range, const int16_t *grid,
                   const double *origin, double res, const double *rot_tab, int reach, int rotations, int min_points,
                   int min_score, int min_gain, int B, int N, int H, int W, double *pose, float *rot, double *trans,
                   int32_t *scores, int32_t *best, int32_t *score, int32_t *votes, uint8_t *ok, uint8_t *moved,
                   double *correction, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N19 grid refine: the pose of a sensor fitted to its own occupancy grid (N12) below the size of a cell.  N13 is a
 * whole-cell search that stays silent while the pose is good; this stage runs every scan and removes the slow drift of a
 * pose composed from scan pairs: a Gauss-Newton fit of the scan's endpoints to the bilinearly interpolated, clamped
 * log-odds, as Hector SLAM does it.  The reference has nothing of the kind; the specification is this comment (restated
 * in NumPy, the order of the sums included, by tests/test_grid_refine.py).  One sensor per batch entry, one launch.
 * Settings: cap in [1, 32767] (32): the count at which a cell is taken as certainly occupied; iters in [1, 32] (8);
 *   min_points >= 0 (50); min_pivot >= 0 (1e-6); max_shift >= 0 in cells (2.0); max_turn >= 0 in radians (0.05);
 *   eps_shift in cells (1e-3); eps_turn in radians (1e-5); max_range and cls_thresh as N13.
 * Inputs: ranges [B][N] float32, the current scan; tab the angle table; optionally the NMS results instance_mask
 *   [B][N], num_det [B] (clamped to [0, N]) and det_cls [B][N], all three or none (NULL); grid [B][H][W] int16 and
 *   origin [B][2] float64 of N12, both read only; res.
 * In/out: pose [B][3] float64 = (x, y, phi), rot [B][4] float32 row-major and trans [B][2] float64, as for N13.
 * A point i VOTES by N13's rule (r finite, 0 < r < max_range, no person's point); V = their number;
 *   p = (r cos_i, r sin_i).  All arithmetic is float64 with plain multiplies and adds (no FMA).
 * Evaluation at (x, y, phi):
 *   (s, c) = sincos(phi) in double -- from the pose, not from the float rot.
 *   d = (c p_x - s p_y, s p_x + c p_y)
 *   u = ((d_x + x) - o_x) / res - 0.5,  v = ((d_y + y) - o_y) / res - 0.5  (true divisions; cell values sit at cell
 *     centres);  i0 = floor(u), j0 = floor(v), f = (u - i0, v - j0).
 *   The point is INSIDE when -1 <= i0 < W and -1 <= j0 < H, compared in double; a NaN is outside.
 *   m(i, j) = (double)clamp(grid[j][i], -cap, cap) / (double)cap, and 0 for a cell outside the grid;
 *     m00, m10, m01, m11 = m at (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1).
 *   M   = (m00 (1 - f_x) + m10 f_x) (1 - f_y) + (m01 (1 - f_x) + m11 f_x) f_y
 *   g_x = (m10 - m00) (1 - f_y) + (m11 - m01) f_y,   g_y = (m01 - m00) (1 - f_x) + (m11 - m10) f_x   (per cell)
 *   l = d / res,  J = (g_x, g_y, g_y l_x - g_x l_y),  e = 1 - M.
 *   Eleven sums over the inside voting points, in the FIXED ORDER of csrc/pof_sensor.h: J_a J_b for ab = 00 01 02 11 12
 *   22 -> A, J_a e -> b, M, and 1 -> n.
 * The fit: the correction (c_x, c_y, c_phi) in cells, cells and radians starts at zero; evaluation k is at
 *   (x_in + c_x res, y_in + c_y res, phi_in + c_phi) -- always the incoming pose plus the accumulated correction.
 *   count = n and s0 = sum M / n of the first evaluation.  An update solves A delta = b by the Cholesky of
 *   csrc/pof_icp.h (pivots tested against min_pivot * dmax as they are formed, obs = the smallest pivot formed over dmax,
 *   of the last solve; 0 before any) and adds delta to the correction.  After `iters` updates, or after an update with
 *   max(|delta_x|, |delta_y|) < eps_shift and |delta_phi| < eps_turn, one more evaluation gives s1 = sum M / n: there
 *   are iters_used + 1 evaluations.
 *   ok    = V >= min_points  and  n >= min_points at every evaluation  and  every pivot passed.  The fit stops at the
 *           first evaluation or solve that fails it.  An empty grid has A = 0 and is not ok.
 *   moved = ok  and  max(|c_x|, |c_y|) <= max_shift  and  |c_phi| <= max_turn  and  s1 > s0.
 * With moved: pose = (x_in + c_x res, y_in + c_y res, phi_in + c_phi), and rot, trans are written from it as
 *   pof_pose_advance writes them.  Without moved pose, rot and trans keep their bits: nothing is stored.
 * Outputs: correction [B][3] float64 = (c_x res, c_y res, c_phi), zeros without moved; score [B][2] float64 = (s0, s1),
 *   s1 NaN when not ok, s0 NaN when count = 0; obs [B] float64; votes [B] int32 = V; count [B] int32; iters_used [B]
 *   int32 = the updates made; ok [B], moved [B] uint8.
 * No atomics, one order of additions: the same bits in every run, at every batch position and in a graph replay.
 * POF_E_BADARG (checked first; nothing written): a NULL pointer other than the three NMS results, NMS pointers given
 *   in part, res not > 0, max_range not > 0, cap outside [1, 32767], iters outside [1, 32], min_points < 0, min_pivot,
 *   max_shift or max_turn not >= 0, B < 0, N < 1.  POF_E_SHAPE (nothing written): N > 4096, H or W not a multiple of 64
 *   or outside [64, 2048].  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_grid_refine(const float *ranges, const double *tab, const int32_t *instance_mask, const int32_t *num_det,
                    const double *det_cls, double cls_thresh, double max_range, const int16_t *grid,
                    const double *origin, double res, int cap, int iters, int min_points, double min_pivot,
                    double max_shift, double max_turn, double eps_shift, double eps_turn, int B, int N, int H, int W,
                    double *pose, float *rot, double *trans, double *correction, double *score, double *obs,
                    int32_t *votes, int32_t *count, int32_t *iters_used, uint8_t *ok, uint8_t *moved,
                    pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N14 scrolling occupancy grid: the grid of N12 follows its sensor.  When the sensor comes within `margin` cells of a
 * border the grid is shifted by whole tiles of 64 cells so that the sensor's tile is the middle tile again -- the tile
 * a reset centres it on -- and what scrolls in is unknown.  The reference has nothing of the kind; the specification
 * is this comment (restated in NumPy by tests/test_grid_scroll.py).  One sensor per batch entry, two launches on the
 * stream (the shifted grid into scratch, then back).
 * State per sensor: N12's grid [B][H][W] int16 and origin [B][2] float64, the origin now WRITTEN by this stage;
 *   persistent base [B][2] float64, the origin as the last reset set it, read only, and offset [B][2] int32, the
 *   cumulative shift in tiles of 64 cells as (x, y); a workspace scratch [B][H][W] int16 whose content means nothing
 *   between calls.
 * Inputs: trans [B][2] float64 (the pose terms' translation), res, margin in cells.
 * Per axis, shown for x with TW = W / 64, float64, plain operations (no FMA):
 *   c_x = floor((t_x - o_x) / res): N12's point_cell arithmetic applied to the sensor position, a true division.
 *   c_x not finite or |c_x| >= 2^30:  s_x = 0.  Otherwise, with the integer c_x and q_x = c_x floor-divided by 64:
 *   s_x = q_x - floor(TW / 2) when c_x < margin or c_x >= W - margin, else 0.
 *   A shift that would make |offset_x + s_x| > 2^20 is not made (s_x = 0).
 *   A triggered scroll puts the sensor's tile back on tile floor(TW / 2), the tile a reset centres it on: the next
 *   scroll is half a grid of travel away.
 * With (s_x, s_y) != (0, 0):  grid'[iy][ix] = grid[iy + 64 s_y][ix + 64 s_x] where that cell exists, else 0 (unknown);
 *   offset += s;  origin = base + (double)(64 offset) res, computed from base and not accumulated: a sensor that scrolls
 *   away and back gets its origin's old bits back, and its cells line up with the old ones exactly.
 * Without a shift grid, origin and offset keep their bits: nothing is stored to them.
 * Outputs: shift [B][2] int32 = (s_x, s_y) and scrolled [B] uint8, both always written.
 * Whole tiles: every row of a 64 x 64 tile stays one 128-byte line, the copy is 16-byte loads and stores in the thread
 *   layout of N12's cells launch, and cell indices move by multiples of 64.
 * No atomics and no sums: the same bits in every run, at every batch position and in a graph replay.
 * POF_E_BADARG (nothing written): a NULL pointer, res not > 0, margin < 0, B < 0 (these are checked first); with H and
 *   W inside N12's rule, margin > 64 floor((TW - 1) / 2) or the same for H -- the bound keeps a re-centred sensor outside
 *   the margin.  POF_E_SHAPE (nothing written): H or W not a multiple of 64 or outside [64, 2048], grid or scratch not
 *   16-byte aligned, B H W / 4096 >= 2^31.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_grid_scroll(const double *trans, double res, int margin, int B, int H, int W, int16_t *grid, double *origin,
                    const double *base, int32_t *offset, int16_t *scratch, int32_t *shift, uint8_t *scrolled,
                    pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N20 tile store behind the scrolling grid: N14's scroll, and what scrolls out of the window is kept per sensor in a
 * store of S = `slots` tiles of 64 x 64 cells, so that a return to a mapped place puts the old cells back under the
 * sensor.  The shift rule and everything N14 writes are N14's, word for word: s_x and s_y, the caps, offset, origin
 * from base, the surviving cells, shift and scrolled.  The reference has nothing of the kind; the specification is
 * this comment (restated in NumPy by tests/test_grid_store.py).  One sensor per batch entry, three launches on the
 * stream (stage, plan, commit).
 * State per sensor beside N14's (grid, origin, base, offset, the workspace scratch), every field persistent and all
 *   zeros after a reset:  store [B][S][64][64] int16;  store_key [B][S][2] int32, the world tile (x, y) a slot holds;
 *   store_stamp [B][S] int32, 0 = the slot is free, else the value of clock at the scroll that wrote it;  clock [B]
 *   int32, the scrolls made since the reset.  Workspaces whose content means nothing between calls: plan_in and
 *   plan_out [B][H / 64 * W / 64] int32.
 * World tile: window tile (tx, ty) under offset o is world tile o + (tx, ty); N14's cap keeps it inside int32.
 * A call with the shift s = (s_x, s_y) != 0, o the offset before it, o' = o + s, TW = W / 64, TH = H / 64:
 *   Arriving tiles: the destination tiles (tx, ty) whose source (tx + s_x, ty + s_y) lies outside the window; world
 *     tile k = o' + (tx, ty).  With a slot j that has store_stamp != 0 and store_key = k -- the lowest such j --
 *     grid'[tile] = store[j] and slot j is RELEASED; otherwise the tile is 0 as in N14.  restored = their number.
 *   Departing tiles: the source tiles (tx, ty) whose destination (tx - s_x, ty - s_y) lies outside the window; world
 *     tile k = o + (tx, ty).  One whose cells are all 0 is not stored (unknown needs no slot); the others are ranked
 *     in ascending tile index ty TW + tx.
 *   Slot order: the effective stamp of a slot is 0 when it was free before the call or is released by it, else its
 *     store_stamp; the slots are ordered by (effective stamp, slot index), ascending -- free slots first, then the
 *     oldest (first in, first out).
 *   Assignment: the r-th ranked departing tile takes the r-th slot of that order, r < S: its 4096 cells are copied
 *     there bit for bit, store_key = k, store_stamp = clock + 1.  stored = the tiles placed, evicted = those among
 *     them whose slot had a non-zero effective stamp, dropped = the ranked tiles with r >= S.
 *   A released slot that nothing took ends with store_stamp = 0.  clock += 1.
 *   A world tile is in the window or in the store, never in both.
 * Without a shift nothing is stored to any state field.
 * Outputs, always written: N14's shift [B][2] int32 and scrolled [B] uint8; counts [B][4] int32 = (restored, stored,
 *   evicted, dropped), zeros without a shift.
 * Integers and bitwise copies, no atomics, no floating point beyond N14's two divisions: the same bits in every run,
 *   at every batch position and in a graph replay.
 * POF_E_BADARG (nothing written): a NULL pointer, slots outside [1, 1024], and N14's.  POF_E_SHAPE (nothing written):
 *   N14's, and a store that is not 16-byte aligned.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_grid_scroll_store(const double *trans, double res, int margin, int slots, int B, int H, int W, int16_t *grid,
                          double *origin, const double *base, int32_t *offset, int16_t *scratch, int16_t *store,
                          int32_t *store_key, int32_t *store_stamp, int32_t *clock, int32_t *plan_in,
                          int32_t *plan_out, int32_t *shift, uint8_t *scrolled, int32_t *counts, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N15 map-checked tracks: per-track evidence from the occupancy grid.  The detection row of the NMS is a rank that
 * changes with every scan and only a track (N7) carries identity over time; this stage joins what the grid (N12) says
 * about the row a track was matched with to the track's slot, sums it there, and derives a class per track: a walker's
 * points land on cells seen free and the track travels, an intermittent false positive on a static object lands on
 * cells the map already holds as occupied.  The reference has nothing of the kind; the specification is this comment
 * (restated in NumPy by tests/test_track_map.py).  One sensor per batch entry, one launch, M = max_tracks.
 * Inputs, read only, as this step's NMS, pof_grid_map_update and pof_track_update left them: instance_mask [B][N],
 *   num_det [B] (clamped to [0, N]), point_cell [B][N] int32, point_prior [B][N] int16, det_points [B][N],
 *   det_free [B][N] int32, track_id [B][M] int32 (0 = free), track_state [B][M][4] float64 = (x, y, vx, vy),
 *   track_det [B][M] int32.
 * State, in place, every field persistent, all zeros after a reset: ev_id [B][M] int32 = the track id the evidence
 *   belongs to; ev_points, ev_free, ev_occ, ev_scans [B][M] int32; ev_start [B][M][2] float64 = where the track stood
 *   when its evidence started; ev_moved [B][M] uint8.
 * One step:
 *   0. per detection row k < num_det:  det_occ[k] = the number of beams i with instance_mask[i] = k + 1,
 *      point_cell[i] >= 0 and point_prior[i] >= occ_thresh (the -32768 of a beam without a cell counts nowhere);
 *      rows >= num_det are 0
 *   1. per slot s, id = track_id[s]:  id = 0: every state field of the slot becomes 0.  Else id != ev_id[s] (the slot
 *      was reused): the fields become 0, ev_id = id and ev_start = (x, y) of track_state[s]
 *   2. per live slot, k = track_det[s]:  if 0 <= k < num_det and n = det_points[k] > 0:  ev_points += n,
 *      ev_free += det_free[k], ev_occ += det_occ[k], ev_scans += 1 (saturating at 2^30); then, if ev_points > cap, the
 *      three sums are each shifted right by one, once: with cap >= N they stay bounded by cap, old evidence fades and
 *      the ratios survive
 *   3. per live slot, float64, plain multiplies and adds (no FMA):  dx = x - ev_start_x, dy = y - ev_start_y,
 *      d2 = dx dx + dy dy;  d2 >= travel travel sets ev_moved = 1, which stays set; a NaN compares false
 *   4. the class of a slot, a pure function of its state, the products in int64:
 *        0 undecided      not live, or ev_scans < min_scans, or ev_points < min_points
 *        3 background     else 100 ev_occ >= occ_pct ev_points  (tested first: a false positive that slides along a
 *                         wall as the sensor moves does travel)
 *        1 free-standing  else ev_moved, or 100 ev_free >= free_pct ev_points
 *        2 unsupported    everything else
 * Outputs, overwritten every step: det_occ [B][N] int32; track_class [B][M] uint8; det_class [B][N] uint8 = the class of
 *   the live slot whose track_det is that row (inside [0, num_det)), else 0 -- should two slots name one row, the
 *   lower slot stands; point_class [B][N] uint8 = det_class[instance_mask - 1] for ids in [1, num_det], else 0;
 *   class_count [B][4] int32 = the live slots per class.
 * Integer sums in LDS, no global and no floating-point atomics: the same bits in every run, at every batch position
 * and in a graph replay.  A grid that scrolls (N14) changes nothing here: the state holds world coordinates and
 * counts, no cells.
 * POF_E_BADARG (checked first; nothing written): a NULL pointer, B < 0, N < 1, max_tracks < 1, occ_thresh < 0, free_pct
 *   or occ_pct outside [0, 100], min_points or min_scans < 0, cap < N or > 2^20, travel not >= 0.  POF_E_SHAPE (nothing
 *   written): N > 4096, max_tracks > 256.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_track_map(const int32_t *instance_mask, const int32_t *num_det, const int32_t *point_cell,
                  const int16_t *point_prior, const int32_t *det_points, const int32_t *det_free,
                  const int32_t *track_id, const double *track_state, const int32_t *track_det, int B, int N,
                  int max_tracks, int32_t *ev_id, int32_t *ev_points, int32_t *ev_free, int32_t *ev_occ,
                  int32_t *ev_scans, double *ev_start, uint8_t *ev_moved, int32_t *det_occ, uint8_t *track_class,
                  uint8_t *det_class, uint8_t *point_class, int32_t *class_count, int occ_thresh, int free_pct,
                  int occ_pct, int min_points, int min_scans, double travel, int cap, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N16 map-predicted scan: a ray cast of the occupancy grid (N12) from the sensor pose, per beam.  N12-N15 read the map
 * only at a beam's endpoint; this stage walks it along the beam and says where the map expects the beam to end, whether
 * the point stands in front of that surface in space the map knows to be empty, whether the beam went through something
 * the map holds as solid, and whether it passed cells the map knows nothing about.  The reference has nothing of the
 * kind; the specification is this comment (restated in NumPy by tests/test_grid_cast.py).  One sensor per batch entry,
 * two launches on the stream (the walk, then the counts).  No state: the grid and the origin are read only, and the
 * grid is read as it stands, so in a step this stage runs in front of pof_grid_map_update, as point_prior is taken.
 * Inputs: ranges [B][N] float32, the current scan; tab the angle table; the pose terms rot [B][4] float32 row-major and
 *   trans [B][2] float64; grid [B][H][W] int16 and origin [B][2] float64 of N12; optionally the NMS results
 *   instance_mask [B][N], num_det [B] (clamped to [0, N]) and det_cls [B][N], all three or none (NULL): only the
 *   detection rows are used, no score gates anything here (det_cls is not read).
 * The walk of beam i, float64 with plain multiplies, adds and true divisions (no FMA, no transcendental):
 *   u_x = (t_x - o_x) / res, u_y likewise; c_x = floor(u_x), c_y = floor(u_y): N14's arithmetic for the sensor's cell.
 *   The sensor is INSIDE when 0 <= c_x < W and 0 <= c_y < H, compared in double (a NaN is outside).  Otherwise every
 *   beam of the sensor has state OUTSIDE and walks nothing.
 *   d_x = (double)R00 cos_i + (double)R01 sin_i,  d_y = (double)R10 cos_i + (double)R11 sin_i.
 *   Crossings of the cell borders on the x axis:  d_x > 0:  a_x = ((c_x + 1.0) - u_x) / d_x, q_x = 1.0 / d_x, step +1;
 *   d_x < 0:  a_x = (u_x - c_x) / (-d_x), q_x = 1.0 / (-d_x), step -1;  otherwise (zero or NaN) the axis has no crossing.
 *   The k-th crossing is at X_k = a_x + (double)k q_x (closed form, no running sum), +inf for an axis without one; the
 *   y axis likewise.  The walk starts in cell (c_x, c_y) with k_x = k_y = 0.
 *   A step:  X = X_kx, Y = Y_ky.  Both +inf: the beam stops (state NONE outside a run).  Else X <= Y:  t = X, the cell
 *   moves by the x step, k_x += 1;  else t = Y, the cell moves by the y step, k_y += 1: through a corner x goes first.
 *   rho = t res: the parameter in cells times res.  (d_x, d_y) is a float32 rotation of a unit vector, so rho is the
 *   metric range along the beam to about 1e-7 relative.  The sensor's own cell is not tested.
 *   For the cell a step enters, in this order:
 *     (a) rho >= max_range: stop; the state is OPEN, or inside an occupied run exp_far = rho and the state stays WALL;
 *     (b) the cell is outside the grid (tested in integers): stop; EDGE, or inside a run exp_far = rho, WALL;
 *     (c) v = grid[iy][ix].  Outside a run and v >= occ_thresh: the run starts, exp_range = rho, exp_cell = iy W + ix,
 *         state WALL, and the walk goes on.  Inside a run and v < occ_thresh: exp_far = rho, stop.  (Walking a run to
 *         its far side keeps a wall seen at a grazing angle, whose cells the beam enters early, from reading as
 *         "gone through".)
 *     (d) the first entered cell with v > -free_thresh, cells of a run included: free_range = rho.
 *   exp_steps = the steps taken, the one that stops the walk included (0 for NONE and OUTSIDE).  A walk ends within
 *   H + W steps: every step moves the cell away from the start by one on one axis, so step H + W at the latest leaves
 *   the grid; no step beyond that is taken and no other bound is relied on.
 * Outputs per beam, [B][N]: exp_range float64 = the range at which the beam enters the first occupied cell, exp_far
 *   float64 = the range at which it leaves that occupied run, both +inf unless the state is WALL; free_range float64 =
 *   the range of the first entered cell not known free, +inf when there was none; exp_cell int32, -1 unless WALL;
 *   exp_state uint8: 0 NONE, 1 OPEN, 2 EDGE, 3 WALL, 4 OUTSIDE; exp_steps int32.
 * The class of point i, r = (double)ranges[i], a HIT by N12's rule (r finite, 0 < r < max_range), tested in this order,
 *   point_class [B][N] uint8:
 *     0 NONE     not a hit, or the state is NONE or OUTSIDE
 *     1 MAP      state WALL and r >= exp_range - tol and r <= exp_far + tol
 *     3 THROUGH  state WALL and r > exp_far + tol
 *     2 NOVEL    r + tol < exp_range and r < free_range: the point stands in front of the map's surface (exp_range is
 *                +inf without one) and every cell the beam passed on the way to it is known free
 *     4 UNKNOWN  everything else
 * Per detection row k < num_det (NMS results given): det_novel, det_map, det_through [B][N] int32 = the points with
 *   instance_mask = k + 1 of class NOVEL, MAP, THROUGH.  Rows >= num_det, and every row without NMS results, are zeros.
 *   class_count [B][5] int32 = the points of the scan per class.
 * Integer sums in LDS, no global and no floating-point atomics: the same bits in every run, at every batch position
 * and in a graph replay.
 * POF_E_BADARG (checked first; nothing written): a NULL required pointer, NMS pointers given in part, res or max_range
 *   not > 0, tol not >= 0, occ_thresh < 1, free_thresh < 0, B < 0, N < 1.  POF_E_SHAPE (nothing written): N > 4096, H or
 *   W not a multiple of 64 or outside [64, 2048], B ceil(N / 64) >= 2^31.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_grid_cast(const float *ranges, const double *tab, const float *rot, const double *trans,
                  const int32_t *instance_mask, const int32_t *num_det, const double *det_cls, const int16_t *grid,
                  const double *origin, double res, double max_range, double tol, int occ_thresh, int free_thresh,
                  int B, int N, int H, int W, double *exp_range, double *exp_far, double *free_range,
                  int32_t *exp_cell, uint8_t *exp_state, int32_t *exp_steps, uint8_t *point_class, int32_t *det_novel,
                  int32_t *det_map, int32_t *det_through, int32_t *class_count, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N17 novelty segments: the NOVEL points of a scan grouped into detections.  N16 says per point whether it stands in
 * front of the map's surface in space the map knows to be empty; this stage turns the runs of such points into
 * detections in the layout every stage behind the detector takes -- instance_mask, num_det, det_xy, det_cls, the results
 * of pof_nms_predicted_center in the argument order of pof_person_motion -- so a mover the net does not report is a
 * detection row all the same, and the chain needs no net at all.  The reference has nothing of the kind; the
 * specification is this comment (restated in NumPy by tests/test_novel_segments.py).  One sensor per batch entry, one
 * launch, the per-sensor workgroup of pof_sensor.h: one wave up to N = 512, 512 threads up to N = 4096, chosen by the
 * launcher from N alone.  No state.
 * Inputs: ranges [B][N] float32, the scan; tab the angle table; point_class [B][N] uint8 as pof_grid_cast writes it (any
 *   byte is legal, only the value 2 means anything); optionally the NMS results nms_instance_mask [B][N], nms_num_det
 *   [B] (clamped to [0, N]) and nms_det_cls [B][N], all three or none (NULL), with cls_thresh: they only feed det_known.
 *   Settings: jump (0.3 m), the largest distance between consecutive members of one segment; max_skip (2), the beams
 *   that may lie between two consecutive members; min_points (3), the fewest members of a kept segment; max_width
 *   (1.0 m), the largest distance between a kept segment's first and last member.
 * Everything is float64 with plain multiplies and adds: no FMA, no libm call, no square root.
 *   MEMBERS.  Beam i is a member when point_class[i] == 2 and r = (double)ranges[i] is finite and r > 0.  Its point is
 *     p_i = (r cos_i, r sin_i), one rounding per product, in the sensor frame.
 *   SEGMENTS.  The members are walked in ascending beam index.  Member i continues the open segment when the previous
 *     member l is at most max_skip beams back, i - l <= max_skip + 1, AND d2 = dx dx + dy dy <= jump jump with dx =
 *     p_i.x - p_l.x, dy = p_i.y - p_l.y and jump jump formed once.  Otherwise i closes the open segment and opens a new
 *     one.  Beams that are no members belong to no segment and do not break one within the skip.  There is no
 *     wrap-around from beam N - 1 to beam 0.
 *   FILTERS, in this order.  A segment with fewer than min_points members is dropped as FEW.  Then w2 = the squared
 *     distance between its last and its first member, d2's expression with i = last and l = first; the segment is
 *     dropped as WIDE unless w2 <= max_width max_width (formed once; written so that a NaN drops it, though members
 *     give none).  A segment that is both counts as few.
 *   ROWS.  The kept segments are numbered in the order of their first beam: row k = 0, 1, ..., instance id k + 1.
 * Outputs, the first four with the dtypes, shapes and meaning of pof_nms_predicted_center's results; every per-row
 *   field is zero in the rows at and beyond num_det:
 *   instance_mask [B][N] int32  k + 1 on the members of kept segment k, else 0
 *   num_det       [B]    int32  the number of kept segments
 *   det_xy     [B][N][2] float64  per row the mean of its members' p, in the sensor frame like the NMS's det_xy: the
 *                                 sums are added in ascending beam index from 0.0 with plain adds, then divided by the
 *                                 count (one true division per coordinate)
 *   det_cls       [B][N] float64  exactly 1.0 on a kept row: a downstream cls_thresh <= 1 passes it
 *   det_count, det_first, det_last [B][N] int32  the row's members, its first and its last beam
 *   det_width2    [B][N] float64  the row's w2
 *   det_known     [B][N] int32  the row's members that belong to a confident NMS detection: nms_instance_mask in [1,
 *                                 nms_num_det] and nms_det_cls[id - 1] >= cls_thresh (pof_person_flow's det_valid);
 *                                 zeros without the NMS results
 *   seg_count     [B][3] int32  segments before the filters, dropped as few, dropped as wide
 * Integer maxima and counts use LDS atomics; every float64 sum is added by one lane in beam order.  No global atomics:
 * the same bits in every run, at every batch position and in a graph replay.
 * POF_E_BADARG (checked first; nothing written): a NULL required pointer, NMS pointers given in part, jump not > 0,
 *   max_width not >= 0, min_points < 1, max_skip outside [0, 64], B < 0, N < 1.  POF_E_SHAPE (nothing written): N >
 *   4096.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_novel_segments(const float *ranges, const double *tab, const uint8_t *point_class,
                       const int32_t *nms_instance_mask, const int32_t *nms_num_det, const double *nms_det_cls,
                       double cls_thresh, double jump, int max_skip, int min_points, double max_width, int B, int N,
                       int32_t *instance_mask, int32_t *num_det, double *det_xy, double *det_cls, int32_t *det_count,
                       int32_t *det_first, int32_t *det_last, double *det_width2, int32_t *det_known,
                       int32_t *seg_count, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N18 merged detections: two detection records made one.  N17's segments and the NMS's rows are both records in the
 * layout of pof_nms_predicted_center's results; the person stages (pof_person_motion, pof_track_update, pof_track_map)
 * and the gate of pof_grid_map_update take one.  This stage appends to the primary record A (the NMS's) the rows of
 * the secondary record B (the segments') that A's confident detections do not already hold, and hands every point to
 * one row.  The reference has nothing of the kind; the specification is this comment (restated in NumPy by
 * tests/test_merge_detections.py).  One sensor per batch entry, one launch, the per-sensor workgroup of pof_sensor.h:
 * one wave up to N = 512, 512 threads up to N = 4096, chosen by the launcher from N alone.  No state.
 * Inputs: B, the secondary record, b_instance_mask [B][N] int32, b_num_det [B] int32, b_det_xy [B][N][2] float64,
 *   b_det_cls [B][N] float64, all required; A, the primary record, a_instance_mask, a_num_det, a_det_xy, a_det_cls of the
 *   same shapes, all four or none (NULL: an empty A).  Settings: cls_thresh; absorb_pct, an int in [0, 101] (50).
 *   nA and nB are a_num_det and b_num_det clamped to [0, N] (nA = 0 without A).
 * Everything is integers and bitwise copies: no floating-point arithmetic except the compare a_det_cls >= cls_thresh.
 *   CONFIDENT.  Point i is confident when its A id a_instance_mask[i] is in [1, nA] and a_det_cls[id - 1] >= cls_thresh
 *     (pof_person_flow's det_valid, the gate of the map stages); a NaN score is not confident.
 *   MEMBERS.  Point i is a member of B row k < nB when b_instance_mask[i] == k + 1; any other id belongs to no row.  Per
 *     B row, b_count[k] is the number of its members and b_known[k] the number of its members that are confident.
 *   ABSORBED.  B row k is absorbed when b_count[k] == 0 or 100 b_known[k] >= absorb_pct b_count[k] (in int32: N <= 4096).
 *     absorb_pct = 0 absorbs every row, absorb_pct = 101 only the empty ones.
 *   ROWS.  Merged rows 0 .. nA - 1 are A's rows, det_xy and det_cls bit for bit (negative zero and NaN payloads
 *     included).  The B rows that are not absorbed are appended in ascending k at the rows nA, nA + 1, ... while the row
 *     index is < N; a row that would land at or beyond N is dropped.  An appended row's det_xy and det_cls are B's, bit
 *     for bit.
 *   MASK.  instance_mask[i] is the appended row + 1 when i is a member of an appended B row and i is not confident;
 *     otherwise a_instance_mask[i] when that is in [1, nA], else 0.  So a confident detection keeps all its points, an
 *     unconfident A row loses the points an appended row claims, and the members of absorbed and dropped rows stay with
 *     A.
 * Outputs, the first four with the dtypes, shapes and meaning of pof_nms_predicted_center's results, in the argument
 *   order of pof_person_motion; every per-row field is zero in the rows at and beyond num_det (b_count and b_known: at
 *   and beyond nB), except b_row, which is -1 at and beyond nB:
 *   instance_mask [B][N] int32  the merged id per point
 *   num_det       [B]    int32  nA + the appended rows
 *   det_xy     [B][N][2] float64, det_cls [B][N] float64  the rows
 *   det_points    [B][N] int32  the points that carry the row's id in the merged mask
 *   det_src       [B][N] uint8  1 = the row is A's, 2 = B's
 *   det_row       [B][N] int32  the row's index in its own record
 *   b_row         [B][N] int32  per B row its merged row; -1 absorbed, -2 dropped
 *   b_count, b_known [B][N] int32  per B row
 *   merge_count   [B][4] int32  nA, appended, absorbed, dropped (the last three sum to nB)
 * Integer counts use LDS atomics; no global atomics: the same bits in every run, at every batch position and in a
 * graph replay.
 * POF_E_BADARG (checked first; nothing written): a NULL required pointer, A pointers given in part, absorb_pct outside
 *   [0, 101], B < 0, N < 1.  POF_E_SHAPE (nothing written): N > 4096.  B = 0 is POF_OK.
 * ---------------------------------------------------------------------- */
int pof_merge_detections(const int32_t *b_instance_mask, const int32_t *b_num_det, const double *b_det_xy,
                         const double *b_det_cls, const int32_t *a_instance_mask, const int32_t *a_num_det,
                         const double *a_det_xy, const double *a_det_cls, double cls_thresh, int absorb_pct, int B, int N,
                         int32_t *instance_mask, int32_t *num_det, double *det_xy, double *det_cls, int32_t *det_points,
                         uint8_t *det_src, int32_t *det_row, int32_t *b_row, int32_t *b_count, int32_t *b_known,
                         int32_t *merge_count, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A12 flow_loss / loss_fn_eval
 *   src/depracted/model/prototype.py:27-32, src/depracted/model/dr_spaam.py:22-27,
 *   src/utils/eval_utils.py:129-134
 * pred/target [B][N][2] float32, mask [B][N] float32 or NULL.
 * epe_sum[b] = sum_i |pred-target| (masked), cnt[b] = number of points counted,
 * aae_sum[b] = sum_i |atan2(p0,p1) - atan2(t0,t1)| (radians); all float64 [B].
 * ---------------------------------------------------------------------- */
int pof_flow_errors(const float *pred, const float *target, const float *mask, int B, int N,
                    double *epe_sum, double *aae_sum, double *cnt, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A9 Prototype._fusion               src/depracted/model/prototype.py:118-156
 * feat1/feat2 [B][C][n] float32 -> out [B][2*max_disp+1][n] float32.
 * ---------------------------------------------------------------------- */
int pof_band_correlation(const float *feat1, const float *feat2, float *out, int B, int C, int n,
                         int kernel_size, int max_disp, pof_stream_t stream);

/* BASELINE config 5 ("fp16 correlation"; no counterpart in the reference, which is float32
 * throughout prototype.py:118-156): the same with float16 feature storage.  Products and
 * accumulation are float32 (a float16 converts exactly), the output stays float32.
 * Alignment (both forms and the backward): none required beyond the element size; feature rows are read with
 * element-aligned loads, so a chunk of a larger batch may start anywhere. */
int pof_band_correlation_f16(const void *feat1_f16, const void *feat2_f16, float *out, int B, int C, int n,
                             int kernel_size, int max_disp, pof_stream_t stream);

/* Backward of pof_band_correlation (training Prototype end to end; in the reference this is torch
 * autograd through the unfold / matmul / gather of src/depracted/model/prototype.py:118-156): given
 * g_out = dL/d out [B][D][n] returns dL/d feat1, dL/d feat2 [B][C][n].  n <= 512. */
int pof_band_correlation_backward(const float *feat1, const float *feat2, const float *g_out,
                                  float *d_feat1, float *d_feat2, int B, int C, int n,
                                  int kernel_size, int max_disp, pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A10 _SpatialAttention.forward (everything after the embedding conv)
 *                                   src/depracted/model/dr_spaam.py:163-217
 * emb_x/emb_t [B][N][E] float32; x/tmpl [B][N][F] float32 (F = channels*pts).
 * band [B][N][w] pre-softmax similarities (clamped duplicates kept),
 * prob [B][N][w] softmax weights with duplicates zeroed (scratch, also useful
 * for the backward pass), out [B][N][F] = alpha*x + (1-alpha)*sum_k prob*tmpl.
 * F % 4 == 0 (POF_E_SHAPE otherwise).  Alignment (forward, f16 form and backward): none required beyond the
 * element size; rows are read and written 4 elements at a time whatever their address (the hardware's unaligned
 * global access), with the same bits as aligned buffers.
 * ---------------------------------------------------------------------- */
int pof_spatial_attention(const float *emb_x, const float *emb_t, const float *x, const float *tmpl,
                          int B, int N, int E, int F, int window, double alpha, float *band,
                          float *prob, float *out, pof_stream_t stream);

/* BASELINE config 5 storage (the reference's dr_spaam.py:163-217 is float32 throughout): the same
 * with the large tensors (x, tmpl, out: [B][N][F]) stored as float16 and float32 arithmetic;
 * the embeddings, band and prob stay float32.  Halves the traffic of the merge kernel. */
int pof_spatial_attention_f16(const float *emb_x, const float *emb_t, const void *x_f16, const void *tmpl_f16,
                              int B, int N, int E, int F, int window, double alpha, float *band, float *prob,
                              void *out_f16, pof_stream_t stream);

/* Backward of pof_spatial_attention (training SpatialDROW through the gate; in the reference torch
 * autograd through src/depracted/model/dr_spaam.py:183-215).
 * g_out = dL/d out [B][N][F]; g_band = dL/d band [B][N][w] or NULL.
 * dsim [B][N][w] is scratch.  Outputs: d_emb_x, d_emb_t [B][N][E]; d_x, d_tmpl [B][N][F]. */
int pof_spatial_attention_backward(const float *emb_x, const float *emb_t, const float *tmpl,
                                   const float *prob, const float *g_out, const float *g_band,
                                   int B, int N, int E, int F, int window, double alpha,
                                   float *dsim, float *d_emb_x, float *d_emb_t, float *d_x,
                                   float *d_tmpl, pof_stream_t stream);

/* The same gradients with the two large passes fused (one walk over g and tmpl: the algorithmic
 * 4 * N * F * 4 bytes instead of reading g and tmpl twice).  workspace:
 * pof_spatial_attention_backward_workspace_bytes(B, N, F, window) bytes of per-column-block partial
 * band products (deterministic: summed in a fixed order by a finishing pass). */
size_t pof_spatial_attention_backward_workspace_bytes(int B, int N, int F, int window);
int pof_spatial_attention_backward_fused(const float *emb_x, const float *emb_t, const float *tmpl,
                                         const float *prob, const float *g_out, const float *g_band,
                                         int B, int N, int E, int F, int window, double alpha,
                                         float *dsim, float *d_emb_x, float *d_emb_t, float *d_x,
                                         float *d_tmpl, void *workspace, size_t workspace_bytes,
                                         pof_stream_t stream);

/* No device work (no HIP call).  Points per lane segment of one call on B <= 65535 scans of N
 * points and F features: forward_segment for the merge walk of pof_spatial_attention(_f16) and the
 * transposed merge of pof_spatial_attention_backward, backward_segment for the fused walk of
 * pof_spatial_attention_backward_fused.  POF_E_BADARG for NULL outputs or sizes < 1, POF_E_SHAPE
 * for F % 4 != 0 or B > 65535. */
int pof_spatial_attention_plan(int B, int N, int F, int *forward_segment, int *backward_segment);

/* ------------------------------------------------------------------------
 * A10 the gate's embedding, inference           src/depracted/model/dr_spaam.py:137-147, :166-171
 * Conv1d(n_channel -> E, kernel_size = n_pts) + BatchNorm1d(eval) + LeakyReLU over whole cutouts,
 * i.e. the dense product with the BatchNorm folded into w and bias:
 *   emb[r][e] = lrelu( sum_k src[r][k] * w[e][k] + bias[e] ),  src in {x, tmpl}
 * x, tmpl [R][K] (K = n_channel * n_pts, contiguous rows), w [E][K] float32 (the folded conv weight as
 * fold_for_inference keeps it), bias [E], emb_x / emb_t [R][E] float32.  tmpl and emb_t may both be NULL
 * (one source).  Both sources go in one launch and share w; no workspace, no memset, no atomics.
 * Shapes: K % 8 == 0, E % 32 == 0, 32 <= E <= 256, R >= 1 (POF_E_SHAPE; sizes < 1 POF_E_BADARG).
 * Alignment: x, tmpl, w, emb_x, emb_t 16-byte aligned, there is no fallback: POF_E_SHAPE otherwise.
 * Every product and sum is float32 on v_mfma_f32_32x32x2_f32, in ONE order for every R and both
 * kernel forms (pof_attn_embed_plan), so a row's result does not depend on the rows it is batched with:
 *   - k in chunks of 8, chunk c on chain c % 4; a chain starts at +0 and takes its chunks in ascending
 *     order, inside a chunk k = 8c + {0, 4, 1, 5, 2, 6, 3, 7}, each step p = fmaf(src[r][k], w[e][k], p);
 *   - s = ((p0 + p1) + p2) + p3;  v = s + bias[e];  emb = v >= 0 ? v : v * (float)negative_slope.
 * ---------------------------------------------------------------------- */
int pof_attn_embed(const float *x, const float *tmpl, long long R, int K, int E, const float *w,
                   const float *bias, double negative_slope, float *emb_x, float *emb_t, pof_stream_t stream);

/* The same on rows stored as IEEE half (float16 storage): a row element is widened in front
 * of its MFMA (exact), so the result is pof_attn_embed on the widened rows, bit for bit.  Same shape
 * and alignment rules, same return codes. */
int pof_attn_embed_f16(const void *x_f16, const void *tmpl_f16, long long R, int K, int E, const float *w,
                       const float *bias, double negative_slope, float *emb_x, float *emb_t, pof_stream_t stream);

/* No device work (no HIP call).  form = 0 for R < 8192: one workgroup per 32 x 32 output tile whose
 * four waves are the four chains and meet in LDS; form = 1 for R >= 8192: one wave per 64 rows x 32
 * columns that carries the four chains of both row tiles in registers.  Same bits either way.
 * POF_E_BADARG for a NULL form or sizes < 1, POF_E_SHAPE for what the launcher refuses as a shape. */
int pof_attn_embed_plan(long long R, int K, int E, int *form);

/* ------------------------------------------------------------------------
 * A13 jump-distance segmentation + per-segment least squares
 *   src/depracted/model/adaboost_person_det.py:71-90 (cuts), :102-210 (features)
 * ranges [B][N] float32.  seg_id [B][N] int32 (segment index of every point),
 * num_seg [B] int32, feat [B][max_seg][16] float64 (columns: see DESIGN.md).
 *
 * max_seg is the number of rows per scan of feat / ref_feat, not a limit on the segmentation.  For a scan
 * with more segments than max_seg:
 *   - num_seg is the true number of segments and seg_id labels every point of the scan, as without a limit;
 *   - feat rows [0, max_seg) are exactly the rows an unlimited call writes (the last one ends at its own
 *     cut, and its jump_next goes to the segment that got no row); nothing is written at or past row max_seg;
 *   - num_kept counts the kept segments (more than two points) among the first max_seg, and ref_feat holds
 *     their rows [0, num_kept): the rows the reference computes from a kept list cut to those segments, so
 *     column 4 is NaN wherever kept[min(q+1, 3)] lies beyond the cut.  Rows from num_kept on are not written.
 * A row the kernel does not write keeps what the caller put there.
 * Coincident points (a run of range 0) leave the normal equations singular; the fit columns then hold the
 * minimum-norm solution the reference's pinv returns (0 for a run of range 0), not NaN.
 * ---------------------------------------------------------------------- */
int pof_segment_features(const float *ranges, const double *tab, int B, int N, double jump_dist,
                         int max_seg, int32_t *seg_id, int32_t *num_seg, double *feat,
                         pof_stream_t stream);

/* The reference's own feature rows, Dataset.scan_to_segments + compute_feature
 *   src/depracted/model/adaboost_person_det.py:71-90, :102-210
 * for the segments it keeps (more than two points, :53-55), in its column order and with its data-set
 * coupled definitions: ref_feat [B][max_seg][15] float64 =
 *   0 n, 1 sigma, 2 ||segment - median||_F / n (:127-130), 3 jump to the previous kept segment,
 *   4 jump to kept[min(q+1, 3)] (:133-138; NaN where the reference raises IndexError), 5 width,
 *   6 line residual, 7 circle criterion, 8 radius, 9 boundary length, 10 boundary regularity,
 *   11 summed curvature, 12 mean angular difference,
 *   13 mean((next_ranges - ranges)[piece q of the unfiltered split] / (odom_dt + 1e-3)) (:196-203),
 *   14 label (+1 when the segment centre lies within radius_wp of an annotation, else -1; :84-88).
 * next_ranges [B][N] (NULL: column 13 = NaN), odom_dt [B] = next_odom - odom (NULL: 0),
 * annotations as CSR wp_offsets [B+1] / wp_xy [W][2] (NULL: every label -1), num_kept [B] (may be NULL).
 * feat (the 16-column table of pof_segment_features) and ref_feat may each be NULL, not both. */
int pof_segment_features_ex(const float *ranges, const float *next_ranges, const double *tab, int B, int N,
                            double jump_dist, const double *odom_dt, const int32_t *wp_offsets,
                            const double *wp_xy, double radius_wp, int max_seg, int32_t *seg_id,
                            int32_t *num_seg, int32_t *num_kept, double *feat, double *ref_feat,
                            pof_stream_t stream);

/* ------------------------------------------------------------------------
 * A16 rotate_iou_gpu_eval                     src/utils/rotate_iou.py:297-404
 * boxes [N][5|7], query [K][5|7] float32 (already permuted to the kernel's
 * x,y,l,w,rot,z,h order for 3-D) -> iou [N][K] float32.
 * Batched form: boxes [G][N][s], query [G][K][s], iou [G][N][K], with optional
 * per-group valid counts n_valid[G], k_valid[G] (NULL = all).
 * ---------------------------------------------------------------------- */
int pof_rotate_iou(const float *boxes, const float *query, float *iou, int G, int N, int K,
                   const int32_t *n_valid, const int32_t *k_valid, int criterion, int is_3d,
                   pof_stream_t stream);

/* ------------------------------------------------------------------------
 * N1: device-resident scan store -> batch of windows.
 *   DROWDataset2.__getitem__ window gather     src/utils/dataset_dr_spaam.py:357-366
 *   scan <-> odometry time association          src/utils/dataset_dr_spaam.py:370-378
 * scans_all [S_total][N] float32: all sequences concatenated.  Per sample b:
 * seq_first[b] = global row of its sequence's first scan, scan_idx[b] = index of the
 * current scan inside the sequence.  out [B][num_scans+1][N]: rows
 * max(0, scan_idx - (num_scans+distance-1-j)*stride), j < num_scans, then scan_idx.
 * row_cur / row_prev [B]: global rows of the current scan and of the last template
 * row (whose time stamps select odom1 / odom0).
 * ---------------------------------------------------------------------- */
int pof_gather_windows(const float *scans_all, const int32_t *seq_first, const int32_t *scan_idx,
                       int B, int num_scans, int distance, int stride, int N, float *out,
                       int32_t *row_cur, int32_t *row_prev, pof_stream_t stream);

/* Scan <-> odometry time association of __getitem__ (src/utils/dataset_dr_spaam.py:369-378):
 * odom{0,1}[b] = odoms[argmin_k |odoms_t[k] - scans_t[row_{prev,cur}[b]]|], k in
 * [odom_lo[b], odom_hi[b]) (the sample's sequence), float32 differences, first
 * minimum wins (np.argmin).  odoms [O_total][3] float32 -> odom0/odom1 [B][3] float64;
 * idx0/idx1 (optional) receive the indices relative to odom_lo. */
int pof_associate_odometry(const float *scans_t, const float *odoms_t, const float *odoms,
                           const int32_t *odom_lo, const int32_t *odom_hi, const int32_t *row_cur,
                           const int32_t *row_prev, int B, double *odom0, double *odom1,
                           int32_t *idx0, int32_t *idx1, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N2 DROW / DR-SPAAM trunk layer, inference     src/depracted/model/dr_spaam.py:8-19, :86-92
 * y = max_pool1d?(LeakyReLU(BatchNorm_eval(Conv1d(k=3, pad=1)(x))), 2) on S sequences:
 * x [S][Ci][L] float32 -> out [S][Co][pool ? L/2 : L].  wt = conv weight transposed to
 * [3][Ci][Co]; scale[Co] = gamma / sqrt(running_var + eps), shift[Co] = beta +
 * (conv_bias - running_mean) * scale (the caller folds them once per checkpoint).
 * Implicit GEMM on the float32 MFMA (exact float32 products, k-ordered accumulation).
 * Alignment (this call, pof_conv1d_bn_lrelu and pof_conv3_first_two): none required beyond 4 bytes; loads and
 * stores are vector-wide whatever the address, with the same bits as aligned buffers.
 * ---------------------------------------------------------------------- */
int pof_conv3_bn_lrelu(const float *x, const float *wt, const float *scale, const float *shift,
                       int S, int Ci, int Co, int L, int pool, double negative_slope, float *out,
                       pof_stream_t stream);

/* Float16 STORAGE through the inference trunk (BASELINE config 5)   src/depracted/model/dr_spaam.py:8-19, :86-92
 * pof_conv3_bn_lrelu with x [S][Ci][L] and out [S][Co][pool ? L/2 : L] as IEEE half.  Weights, scale and
 * shift stay float32 and so does every product and sum, on the same kernel form, sequence chunks and
 * summation order as the float32 call of that shape (pof_conv1d_plan): the result is
 * pof_conv3_bn_lrelu on the widened input, rounded once to nearest even (after the pooled maximum),
 * bit for bit -- overflow to +-inf, float16 subnormals kept on input and output.  Same shape rules and
 * return codes.  Alignment: none required beyond 2 bytes. */
int pof_conv3_bn_lrelu_f16(const void *x_f16, const float *wt, const float *scale, const float *shift,
                           int S, int Ci, int Co, int L, int pool, double negative_slope, void *out_f16,
                           pof_stream_t stream);

/* The same layer with kernel_size 1 or 3 (padding kernel_size / 2) and stride 1 or 2 (round 3): the units of the
 * Prototype flow network -- Conv1d(k = 3, stride 2 | 1) / Conv1d(k = 1) + BatchNorm(eval) + LeakyReLU --
 * src/depracted/model/prototype.py:6-25, 38-45.  wt [kernel_size][Ci][Co]; out [S][Co][Lc] with
 * Lc = L (stride 1) or (L + 1) / 2 (stride 2), halved again when pool != 0 (stride 1 only, Lc even).
 * Supported: (3, 1), (3, 2), (1, 1); anything else returns POF_E_SHAPE. */
int pof_conv1d_bn_lrelu(const float *x, const float *wt, const float *scale, const float *shift,
                        int S, int Ci, int Co, int L, int kernel_size, int stride, int pool,
                        double negative_slope, float *out, pof_stream_t stream);

/* No device work (no HIP call at all: it answers on a machine without a GPU).  The kernel form
 * pof_conv3_bn_lrelu (kernel_size 3, stride 1), pof_conv1d_bn_lrelu or, with fused_first != 0,
 * pof_conv3_first_two (Ci = C1) would launch for these sizes: split_k (1: the
 * four waves of a workgroup share one column tile and split the K loop), channels_per_workgroup (32,
 * 64 or 128), both of the first launch; launches (sequences go in chunks of < 2^30 input elements,
 * and a smaller last chunk may take a narrower form); wide_offsets = how many launches write at
 * least 2^30 output elements (64-bit output offsets).  POF_E_BADARG for NULL outputs or sizes < 1,
 * POF_E_SHAPE for what the launchers refuse as a shape. */
int pof_conv1d_plan(int S, int Ci, int Co, int L, int kernel_size, int stride, int pool, int fused_first,
                    int *split_k, int *channels_per_workgroup, int *launches, int *wide_offsets);

/* ----------------------------------------------------------------------
 * N2 detector heads, inference                  src/depracted/model/dr_spaam.py:104-121
 * pred_cls[s][o] = b_cls[o] + sum_c w_cls[o][c] * mean_l feat[s][c][l]   (o < n_cls <= 6)
 * pred_reg[s][o] = b_reg[o] + sum_c w_reg[o][c] * mean_l feat[s][c][l]   (o < 2)
 * -- the average pool over the last block's positions and the two 1x1 convolutions
 * (conv_cls [n_cls][C][1], conv_reg [2][C][1]) in one launch.  feat [S][C][L] float32.
 * ---------------------------------------------------------------------- */
int pof_drow_heads(const float *feat, int S, int C, int L, const float *w_cls, const float *b_cls,
                   int n_cls, const float *w_reg, const float *b_reg, float *pred_cls,
                   float *pred_reg, pof_stream_t stream);

/* The same heads on feat [S][C][L] as IEEE half (float16 storage of the trunk, src/depracted/model/dr_spaam.py:104-121):
 * widened exactly as it is read, sums and outputs float32 -- the bits of pof_drow_heads on the widened feat. */
int pof_drow_heads_f16(const void *feat_f16, int S, int C, int L, const float *w_cls, const float *b_cls,
                       int n_cls, const float *w_reg, const float *b_reg, float *pred_cls,
                       float *pred_reg, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N2 trunk unit tail, training                  src/depracted/model/dr_spaam.py:8-19, :86-92
 * z = max_pool1d?(LeakyReLU(BatchNorm1d_train(y)), 2) and its backward pass, for the
 * convolution output y [S][C][L] float32 (L <= 256, C*L % 4 == 0, L even when pooled):
 * out [S][C][pool ? L/2 : L].  Batch statistics over (S, L) in float64; running_mean /
 * running_var (may be NULL) are updated with `momentum` as torch.nn.BatchNorm1d does
 * (unbiased variance); save_mean / save_invstd [C] are what the backward pass needs
 * besides y.  backward: dz [S][C][L or L/2] -> dy [S][C][L], dgamma [C], dbeta [C]; the
 * pool routes a gradient to the first maximum of its pair (torch.max_pool1d).
 * dbias_in [C] (may be NULL) = sum of dy over (S, L): the gradient of a per-channel bias
 * added in front of the BatchNorm (the convolution's), from the same pass that writes dy.
 * groups >= 1 (S % groups == 0): the sequences form `groups` equal contiguous ranges, each
 * normalised with its OWN batch statistics -- the five scans of a DR-SPAAM window, which the
 * reference sends through the trunk one after the other (dr_spaam.py:246-262), in one launch;
 * save_mean / save_invstd are then [groups][C] and the running statistics receive the groups'
 * updates in order, as `groups` separate calls would give.
 * workspace: pof_bn_lrelu_pool_workspace_bytes(S, C, L, groups) bytes (0 = unsupported shape).
 * Alignment: none required beyond 4 bytes (float4 accesses at any address, same bits as aligned buffers).
 * ---------------------------------------------------------------------- */
size_t pof_bn_lrelu_pool_workspace_bytes(long long S, int C, int L, int groups);
int pof_bn_lrelu_pool_forward(const float *y, long long S, int C, int L, int groups, const float *gamma,
                              const float *beta, float *running_mean, float *running_var,
                              double momentum, double eps, double negative_slope, int pool,
                              float *out, float *save_mean, float *save_invstd, void *workspace,
                              size_t workspace_bytes, pof_stream_t stream);
int pof_bn_lrelu_pool_backward(const float *y, const float *dz, long long S, int C, int L, int groups,
                               const float *gamma, const float *beta, const float *save_mean,
                               const float *save_invstd, double negative_slope, int pool, float *dy,
                               float *dgamma, float *dbeta, float *dbias_in, void *workspace,
                               size_t workspace_bytes, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N2 trunk unit tail, training, GLOBAL-batch statistics             SURVEY 8(e)
 * (no reference site: the reference has no data parallelism.)  The tail above cut in two at
 * the per-channel sums, so that the ranks of a data-parallel job can add theirs between the
 * calls; everything else -- shapes, pool modes, groups, workspace size
 * (pof_bn_lrelu_pool_workspace_bytes of the LOCAL S), alignment -- is as above.  Exchange
 * buffers, float64, one all-reduce(sum) each:
 *   stat [groups][2C + 1] = sum y [C] | sum y^2 [C] | count (= S / groups * L, written by the kernel)
 *   red  [groups][2C]     = sum dU [C] | sum dU * xhat [C]      (undivided)
 * pof_bn_sync_forward_stats:   y -> stat (this rank's sums and count).
 * pof_bn_sync_forward_apply:   stat (summed over the ranks) -> save_mean / save_invstd [groups][C]
 *   (mean and biased variance over the global count), running statistics updated with the
 *   unbiased variance over the global count, once per group in order; out as in the one-shot form.
 * pof_bn_sync_backward_reduce: y, dz -> red (this rank's sums), dgamma / dbeta [C] of THIS rank's
 *   samples (a gradient all-reduce averages them like every other parameter gradient).
 * pof_bn_sync_backward_apply:  red (summed over the ranks) and stat (for the global count) ->
 *   dy [S][C][L]; dbias_in [C] (may be NULL) = this rank's sum of dy over (S, L).
 * With exchange buffers left as the first call of each pair wrote them (one rank), out,
 * save_mean, save_invstd, the running statistics, dy, dgamma, dbeta and dbias_in have the bits
 * of pof_bn_lrelu_pool_forward / _backward.
 * ---------------------------------------------------------------------- */
int pof_bn_sync_forward_stats(const float *y, long long S, int C, int L, int groups, double *stat,
                              void *workspace, size_t workspace_bytes, pof_stream_t stream);
int pof_bn_sync_forward_apply(const float *y, long long S, int C, int L, int groups, const double *stat,
                              const float *gamma, const float *beta, float *running_mean,
                              float *running_var, double momentum, double eps, double negative_slope,
                              int pool, float *out, float *save_mean, float *save_invstd,
                              void *workspace, size_t workspace_bytes, pof_stream_t stream);
int pof_bn_sync_backward_reduce(const float *y, const float *dz, long long S, int C, int L, int groups,
                                const float *gamma, const float *beta, const float *save_mean,
                                const float *save_invstd, double negative_slope, int pool, double *red,
                                float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                pof_stream_t stream);
int pof_bn_sync_backward_apply(const float *y, const float *dz, long long S, int C, int L, int groups,
                               const float *gamma, const float *beta, const float *save_mean,
                               const float *save_invstd, const double *red, const double *stat,
                               double negative_slope, int pool, float *dy, float *dbias_in,
                               void *workspace, size_t workspace_bytes, pof_stream_t stream);

/* The trunk's first TWO units in one launch (inference): x [S][L] float32 is the single-channel
 * cutout (dr_spaam.py:86-92, conv_block_1[0] and [1]); the C1 channels of the first unit,
 * lrelu_slope1(a0 x[q-1] + a1 x[q] + a2 x[q+1] + b) with l1[c] = {a0, a1, a2, b} (its taps times its
 * folded BatchNorm scale, and its shift; zero padding at the sequence borders), are computed inside
 * the second unit's kernel instead of being written and read back (1 GB each way at B = 32).  wt
 * [3][C1][Co], scale / shift [Co], pool, negative_slope: the second unit, as in pof_conv3_bn_lrelu.
 * C1 <= 128.  The first unit's sums are FMA chains here and MFMA accumulations in the two-launch
 * form: results agree to float32 round-off, not bit for bit. */
int pof_conv3_first_two(const float *x, const float *l1, double slope1, const float *wt, const float *scale,
                        const float *shift, int S, int C1, int Co, int L, int pool, double negative_slope,
                        float *out, pof_stream_t stream);

/* pof_conv3_first_two in float16 storage (dr_spaam.py:86-92, conv_block_1[0] and [1]): x [S][L] is the
 * float16 cutout (pof_cutout_f16), out [S][Co][pool ? L/2 : L] half; l1, wt, scale and shift float32.
 * Equal to pof_conv3_first_two on the widened cutout, rounded once to nearest even, bit for bit; same
 * shape rules and return codes.  There is no mixed in / out form. */
int pof_conv3_first_two_f16(const void *x_f16, const float *l1, double slope1, const float *wt,
                            const float *scale, const float *shift, int S, int C1, int Co, int L, int pool,
                            double negative_slope, void *out_f16, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N2 trunk convolution, weight gradient         src/depracted/model/dr_spaam.py:8-19
 * dw[co][ci][t] = sum_{s,l} dy[s][co][l] * x[s][ci][l + t - 1]  (Conv1d k = 3, pad = 1):
 * x [S][Ci][L], dy [S][Co][L] float32 -> dw [Co][Ci][3] float32 (torch's weight layout).
 * Split-K float32-MFMA GEMM over (sequence, position), deterministic (partial tiles in
 * the workspace, one reduction pass).  The forward and the data gradient of the same
 * convolution are pof_conv3_bn_lrelu with unit scale / slope 1 (data gradient: dy as
 * input, taps reversed, channel roles swapped).
 * workspace: pof_conv3_wgrad_workspace_bytes(S, Ci, Co, L) bytes (0 = unsupported shape: rows longer
 * than 64 positions, or odd rows longer than 32 -- callers keep their library path for those).
 * ---------------------------------------------------------------------- */
size_t pof_conv3_wgrad_workspace_bytes(int S, int Ci, int Co, int L);
int pof_conv3_wgrad(const float *x, const float *dy, int S, int Ci, int Co, int L, float *dw,
                    void *workspace, size_t workspace_bytes, pof_stream_t stream);
/* The same pass for kernel_size 1 | 3 (1: the point-wise convolutions of the box-regression PointNet,
 * src/model/box_regression.py:8-17, and of the Prototype head, src/depracted/model/prototype.py:52-58):
 * dw [Co][Ci][kernel_size]; kernel_size 3 is pof_conv3_wgrad.
 * Alignment: the load width is 4 / 2 / 1 floats by L % 4, L % 2 when x and dy are both 16-byte aligned, 1 float
 * otherwise.  The workspace size and the shapes supported are those of 16-byte aligned operands: with an unaligned
 * x or dy a supported shape may return POF_E_SHAPE (rows of more than 32 floats) or POF_E_WORKSPACE (the split
 * doubles).  Callers hand the kernel aligned copies (ops.conv3_wgrad does). */
size_t pof_conv1d_wgrad_workspace_bytes(int S, int Ci, int Co, int L, int kernel_size);
int pof_conv1d_wgrad(const float *x, const float *dy, int S, int Ci, int Co, int L, int kernel_size, float *dw,
                     void *workspace, size_t workspace_bytes, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * configs[3] box-regression head, dense layers    src/model/box_regression.py:26-45 (_fc), :139-141
 * out[b][n] = sum_k x[b][k] * w[n][k] + bias[n] (torch.nn.Linear's forward; x [B][K], w [N][K],
 * bias [N] or NULL, out [B][N], float32, K a multiple of 4, x and w 16-byte aligned: POF_E_SHAPE
 * otherwise, no fallback -- ops.linear_bias copies unaligned operands; bias and out may be anywhere).  For the
 * head's batch (a few hundred rows): one workgroup per 32 x 32 output tile, K split over its
 * four waves, float32 MFMA, deterministic.  The backward GEMMs stay with the BLAS library.
 * ---------------------------------------------------------------------- */
int pof_linear_bias(const float *x, const float *w, const float *bias, int B, int K, int N, float *out,
                    pof_stream_t stream);

/* ----------------------------------------------------------------------
 * configs[3] box-regression loss                   src/model/box_regression.py:52-67 (regression_loss2)
 * pred, target [B][T] float32, T = 3 (dims, dims, orientation) or 5 (z, 3 dims, orientation):
 * loss[0] = mean_b sum_j c_j |pred - target|, c_j = 1 except c_{T-1} = alpha; dpred [B][T] (or
 * NULL) = d loss / d pred = c_j sign(pred - target) / B.  One launch instead of the ~27 the
 * composed form takes forward and backward.
 * ---------------------------------------------------------------------- */
int pof_regression_loss2(const float *pred, const float *target, long long B, int T, double alpha, float *loss,
                         float *dpred, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N3 BoxRegressor input preparation, batched     box_regressor.py:43-75, :94-105
 *                                                src/data_handle/jrdb_handle.py:178-256
 * points [Np][D] float64 (D = 2 or 3), centers [S][D], oris [S] -> per detection the
 * radius query norm(points - centre) <= radius (float64), count[S] = segment size,
 * and x [S][input_size][D+1] float32 = the reference's fixed-size resampling
 * (random subset when larger, repeat + pad when smaller) of (point - centre, ori).
 * Segments with fewer than min_segment_size points get zero rows (the caller skips
 * them, as the reference returns None).  Randomness: a counter-based hash of
 * (seed, detection index, point index); rows come out in hash order (the consumer is
 * order invariant; the reference's order depends on the global NumPy RNG).
 * mask (optional, [S][Np] uint8) receives the radius-query result itself
 * (generate_segment / anns_to_segments return the variable-size segment).
 * ---------------------------------------------------------------------- */
int pof_segment_inputs(const double *points, int Np, int D, const double *centers, const double *oris,
                       int S, double radius, int input_size, int min_segment_size, uint32_t seed,
                       float *x, int32_t *count, uint8_t *mask, pof_stream_t stream);

/* Training-side twin (src/data_handle/jrdb_dataset.py:99-156): segments already cut (CSR
 * seg_offsets [S+1] over points [P][D]); per sample: subtract centers[s], optionally append
 * extra[s] as a column (the random input angle), optionally drop int(n * random_drop) random
 * points first, then the same fixed-size resampling -> x [S][input_size][D + (extra ? 1 : 0)],
 * count[s] = points kept.  max_segment = longest segment (<= 4096). */
int pof_segment_resample(const double *points, int D, const int32_t *seg_offsets, int S, int max_segment,
                         const double *centers, const double *extra, double random_drop, int input_size,
                         uint32_t seed, float *x, int32_t *count, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N4 scans_to_polar_grid                        src/utils/utils.py:492-531
 * scans [B][T][N] float32 -> out [B][T][R][N] float32, R = int((max-min)/bin) + 1:
 * the truncated-signed-distance column of every beam (the "fc2d" network input,
 * src/utils/dataset_dr_spaam.py:455-458).  float32 arithmetic as NumPy >= 2 evaluates
 * the reference (bit-exact against it); tsdf_clip <= 0 disables the distance ramp.
 * Alignment: none required.  The flat kernel (16-byte stores) runs when out is 16-byte aligned and
 * N * 8 + (2R + 1) * 4 <= 60 KB; otherwise 4 points per lane with float4 accesses when N % 4 == 0 and scans and
 * out are 16-byte aligned, else 1 point per lane.  All three give the same bits.
 * ---------------------------------------------------------------------- */
int pof_polar_grid(const float *scans, int B, int T, int N, double min_range, double max_range,
                   double range_bin_size, double tsdf_clip, int normalize, float *out,
                   pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N1, host side: numeric CSV -> float64 matrix (no device work, no stream).
 * Replaces np.genfromtxt(path, delimiter=",") for the DROW sequence files
 * (src/utils/dataset_dr_spaam.py:473-478 `.csv`, :504-509 `.odom2`, :497-502
 * `.difodom`; bin/data_prepare.py:70-72 `.flow`).  Fields are converted with
 * strtod (correctly rounded, = Python float()); blank lines and `#` lines are
 * skipped, empty / unparsable fields become NaN.  pof_csv_shape reports the
 * row count and the column count of the first row; pof_csv_read_f64 fills a
 * caller-owned [rows][cols] buffer (POF_E_SHAPE if the file does not have
 * exactly that shape on every row); threads <= 0: one per hardware thread (max 16).
 * ---------------------------------------------------------------------- */
int pof_csv_shape(const char *path, long long *rows, int *cols);
int pof_csv_read_f64(const char *path, long long rows, int cols, double *out, int threads);

/* ----------------------------------------------------------------------
 * N4: boosted decision stumps of the legacy person-detection baseline.
 * pof_stump_search replaces BoostedFeatureDetector.simple_classifier
 * (src/depracted/model/adaboost_person_det.py:283-347) for all D feature
 * dimensions in one launch: X [rows][D] float64, Y [rows] (+1 / -1), the n
 * samples are rows index[0..n) (index NULL: rows 0..n-1; 2 <= n <= 2048,
 * duplicates allowed -- the boosting loop samples with replacement).  Per
 * dimension d: n_thresh[d] = number of threshold candidates (midpoints of
 * sorted neighbours of opposite class), min_err[d] / max_err[d] = smallest /
 * largest count of samples misclassified by "x > theta -> +1" over the
 * candidates, theta_min[d] / theta_max[d] = the FIRST candidate (ascending)
 * reaching it (-1 / 0.0 when there is no candidate).  Equal feature values
 * keep their sample order (the reference's np.argsort leaves that order to the
 * sort implementation).  X must be finite.
 * pof_stump_vote replaces BoostedFeatureDetector.eval (:349-378): result[i] =
 * sum_k alpha[k] * (X[i][dim[k]-1] > theta[k] ? +1 : -1) accumulated in k order
 * in float64, label[i] = sign(result[i]) (label may be NULL); dim is 1-based,
 * 0 addresses the last column (an unused round of the reference's K x 2
 * parameter table).
 * ---------------------------------------------------------------------- */
int pof_stump_search(const double *X, const double *Y, long long rows, const int *index, int n, int D,
                     int *min_err, double *theta_min, int *max_err, double *theta_max, int *n_thresh,
                     pof_stream_t stream);
int pof_stump_vote(const double *X, long long N, int D, const int *dim, const double *theta,
                   const double *alpha, int K, double *result, double *label, pof_stream_t stream);

/* ----------------------------------------------------------------------
 * N4, host side: LZF block decoder for `DATA binary_compressed` .pcd files.
 * Replaces lzf.decompress(compressed_data, uncompressed_size) in the vendored
 * pypcd (src/data_handle/_pypcd.py:249-264), which JRDBHandle._load_pointcloud
 * (src/data_handle/jrdb_handle.py:293-305) goes through.  Returns the number of
 * bytes written to out, or -1 when the stream is malformed, refers before the
 * start of the output or would exceed out_cap (nothing outside [out, out+out_cap)
 * is touched).
 * ---------------------------------------------------------------------- */
long long pof_lzf_decompress(const void *in, long long in_len, void *out, long long out_cap);

#ifdef __cplusplus
}
#endif
#endif /* POF_ABI_H */
