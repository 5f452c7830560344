// N8: the sensor's own motion between two consecutive scans without a flow field -- a point-to-line ICP of the
// current scan against the previous one, one launch per batch, one scan pair per workgroup.  On a static scene the
// result inverts get_displacement_from_odometry (src/utils/utils.py:639-662); it has the (theta, u) convention of
// pof_ego_motion's rigid model (a point now at p was at R(theta) p + u), so pof_pose_advance takes it unchanged.
// The reference has no scan matcher: the specification is this comment and that of pof_icp.h, restated in
// float64 NumPy by tests/test_scan_match.py (match_oracle).
//
// Points.  a_j = r_prev[j] * (cos, sin)[j], p_i = r_cur[i] * (cos, sin)[i] in float64 from the angle table, as
// rphi_to_xy.  A range is valid when it is finite and < max_range.  A current point is also left out when it belongs
// to a detection of score >= cls_thresh (instance_mask, num_det, det_cls as in pof_ego_motion; people do not vote).
// dphi = tab[1] - tab[0] (0 for N = 1).  Start: (theta, u) = init row, zeros when init is NULL or the row has a
// component that is not finite.  gate2 = gate * gate, gap2 = max_gap * max_gap.
//
// Correspondence, one iteration and the pass afterwards that writes corr / flow_residual: pof_icp.h, shared with
// pof_keyframe_match.  The window of point i is centred on the beam i + shift:
//   shift = (int)clamp(rint(theta / dphi), -N, N)   (0 when dphi == 0; a NaN quotient gives -N)
// A failed pair: ok = 0, motion and rms NaN, corr -1, flow_residual NaN.
//
// The previous scan's vertices are staged once in LDS, the current points stay in registers, every sum has a FIXED
// ORDER (pof_icp.h).  N <= 512: one wave per pair;   N <= 4096: 512 threads per pair.
// init may be the motion buffer: a workgroup reads its row before it writes it.
#include "pof_icp.h"

namespace {

using namespace pof_icp;

// ranges_prev first and init behind N: with the inputs in another order the 512-thread form measured 2 % slower
struct ScanMatchArgs {
    const float *ranges_prev;
    Input in;
    Settings set;
    int N;
    const double *init;
    double *motion;
    int32_t *count;
    double *rms;
    uint8_t *ok;
    int32_t *iters_used;
    double *obs;
    int32_t *corr;
    double *flow_residual;
};

__device__ __forceinline__ int beam_shift(double th, double dphi, int N)
{
    if (dphi == 0.0) return 0;
    double t = rint(th / dphi);
    if (!(t >= (double)-N)) t = (double)-N;
    if (!(t <= (double)N)) t = (double)N;
    return (int)t;
}

// the window of point i is centred on beam i + shift(theta)
struct ShiftCentre {
    double dphi;
    int N, shift;
    __device__ __forceinline__ void set(double th) { shift = beam_shift(th, dphi, N); }
    __device__ __forceinline__ int operator()(int i, double, double) const { return i + shift; }
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void scan_match_kernel(ScanMatchArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ double s_ax[kMaxN], s_ay[kMaxN];
    __shared__ double s_part[kSums * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, b = blockIdx.x;
    const double qnan = __builtin_nan("");

    double px[kSlots], py[kSlots];
    bool valid[kSlots];
    stage<THREADS>(a.in, a.ranges_prev, b, N, s_ax, s_ay, px, py, valid);
    ShiftCentre centre = {N > 1 ? a.in.tab[1] - a.in.tab[0] : 0.0, N, 0};
    Pose m = {0.0, 0.0, 0.0, 1.0, 0.0};
    if (a.init) {
        const double t0 = a.init[3 * b], t1 = a.init[3 * b + 1], t2 = a.init[3 * b + 2];
        if (isfinite(t0) && isfinite(t1) && isfinite(t2)) {
            m.th = t0;
            m.ux = t1;
            m.uy = t2;
        }
    }
    __syncthreads();                                           // the vertices are staged; init is read

    const Result r = iterate<THREADS>(s_ax, s_ay, s_part, N, a.set, centre, px, py, valid, m);
    write_corr<THREADS>(s_ax, s_ay, b, N, a.set, centre, px, py, valid, m, r.failed, a.corr, a.flow_residual);
    if (threadIdx.x == 0) {
        a.motion[3 * b] = r.failed ? qnan : m.th;
        a.motion[3 * b + 1] = r.failed ? qnan : m.ux;
        a.motion[3 * b + 2] = r.failed ? qnan : m.uy;
        a.count[b] = r.matched;
        a.rms[b] = r.failed ? qnan : r.rms;
        a.ok[b] = r.failed ? 0 : 1;
        a.iters_used[b] = r.used;
        a.obs[b] = r.obs;
    }
}

}  // namespace

extern "C" int pof_scan_match(const float *ranges_prev, const float *ranges_cur, const double *tab, const double *init,
                              const int32_t *instance_mask, const int32_t *num_det, const double *det_cls,
                              double cls_thresh, double max_range, int window, double gate, double max_gap,
                              double huber_delta, int iters, double eps_theta, double eps_u, double min_pivot, int B,
                              int N, double *motion, int32_t *count, double *rms, uint8_t *ok, int32_t *iters_used,
                              double *obs, int32_t *corr, double *flow_residual, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges_prev || !ranges_cur || !tab || !motion || !count || !rms || !ok || !iters_used || !obs)
        return POF_E_BADARG;
    if (check_settings(window, gate, max_gap, huber_delta, iters, instance_mask, num_det, det_cls, B, N) != POF_OK)
        return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_ego_motion and the NMS
    if (B == 0) return POF_OK;
    ScanMatchArgs a;
    a.in = {ranges_cur, tab, {instance_mask, num_det, det_cls, cls_thresh}, max_range};
    a.set = {gate * gate, max_gap * max_gap, huber_delta, eps_theta, eps_u, min_pivot, window, iters};
    a.ranges_prev = ranges_prev; a.init = init; a.N = N;
    a.motion = motion; a.count = count; a.rms = rms; a.ok = ok; a.iters_used = iters_used; a.obs = obs; a.corr = corr;
    a.flow_residual = flow_residual;
    POF_LAUNCH_PER_SENSOR(scan_match_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
