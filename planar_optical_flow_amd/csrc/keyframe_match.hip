// N9: keyframe scan matching -- the current scan is matched against a reference scan (the keyframe) that stays fixed
// until the sensor has moved away from it, and the pose is key_pose o (theta, u): no fit error accumulates while one
// keyframe is held.  One launch per batch, one sensor per workgroup; the keyframe, its pose, the last good match, the
// bookkeeping and the pose are persistent state updated in place, so a captured step stays one linear chain with no
// host decision.  The reference has no scan matcher: the specification is the N9 comment of include/pof_abi.h,
// restated in float64 NumPy by tests/test_keyframe.py (keyframe_oracle).  This file states only what differs from
// pof_scan_match (scan_match.hip): the gate, line partner, normal, residual, Huber weight, sums, solve, composition
// and stop rule are the one copy in pof_icp.h that both use.
//
// Window centre.  The keyframe may be tens of beams away from the current scan in every direction, so the window of a
// point is centred on the beam its transformed position falls on:
//   q = R(theta) p + u,  mid = (int)clamp(rint((atan2(q_y, q_x) - tab[0]) / dphi), -N, 2N)
// (0 when dphi == 0, -N for a NaN), searched over [mid - W, mid + W] n [0, N) upwards with a strict <.  No wrap-around.
//
// One step: see the header.  A workgroup reads its key_ranges row only while staging (before the first barrier) and
// every thread writes only the beams it staged itself, after the last correspondence pass: the replacement is in
// place.  The scalar state of a sensor is read by every thread before the first barrier and written by thread 0 at the
// end.
//
// As scan_match.hip: the keyframe's vertices staged once in LDS, the current points in registers, every sum in a FIXED
// ORDER (pof_icp.h) plus one, before the loop, that counts the current points that vote.
// N <= 512: one wave per sensor;  N <= 4096: 512 threads per sensor.
#include "pof_icp.h"

namespace {

using namespace pof_icp;

struct KeyframeArgs {
    Input in;
    Settings set;
    double key_rot, key_dist2, min_share;
    int max_misses, N;
    float *key_ranges;
    double *key_pose, *key_rel;
    uint8_t *key_valid;
    int32_t *key_age, *key_misses;
    double *pose;
    double *motion;
    int32_t *count;
    double *rms;
    uint8_t *ok;
    int32_t *iters_used;
    double *obs;
    uint8_t *key_replaced;
    int32_t *corr;
    double *flow_residual;
    float *rot;
    double *trans, *flow_trans;
};

// the beam the point q falls on; phi0 = tab[0]
__device__ __forceinline__ int beam_of(double qx, double qy, double phi0, double dphi, int N)
{
    if (dphi == 0.0) return 0;
    double t = rint((atan2(qy, qx) - phi0) / dphi);
    if (!(t >= (double)-N)) t = (double)-N;
    if (!(t <= (double)(2 * N))) t = (double)(2 * N);
    return (int)t;
}

// the window of a point is centred on the beam its transformed position q falls on
struct BeamCentre {
    double phi0, dphi;
    int N;
    __device__ __forceinline__ void set(double) {}
    __device__ __forceinline__ int operator()(int, double qx, double qy) const
    {
        return beam_of(qx, qy, phi0, dphi, N);
    }
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void keyframe_match_kernel(KeyframeArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ double s_ax[kMaxN], s_ay[kMaxN];
    __shared__ double s_part[kSums * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const double qnan = __builtin_nan("");
    const float qnanf = __builtin_nanf("");

    double px[kSlots], py[kSlots];
    bool valid[kSlots];
    double votes[1] = {stage<THREADS>(a.in, a.key_ranges, b, N, s_ax, s_ay, px, py, valid)};
    const double phi0 = a.in.tab[0];
    BeamCentre centre = {phi0, N > 1 ? a.in.tab[1] - phi0 : 0.0, N};
    // the sensor's state, the same values in every thread
    const bool seeded = a.key_valid[b] != 0;
    const double x_old = a.pose[3 * b], y_old = a.pose[3 * b + 1], phi_old = a.pose[3 * b + 2];
    const double kx = a.key_pose[3 * b], ky = a.key_pose[3 * b + 1], kphi = a.key_pose[3 * b + 2];
    const int age = a.key_age[b], misses = a.key_misses[b];
    Pose m = {0.0, 0.0, 0.0, 1.0, 0.0};
    {
        const double t0 = a.key_rel[3 * b], t1 = a.key_rel[3 * b + 1], t2 = a.key_rel[3 * b + 2];
        if (isfinite(t0) && isfinite(t1) && isfinite(t2)) {
            m.th = t0;
            m.ux = t1;
            m.uy = t2;
        }
    }
    __syncthreads();                                           // the vertices are staged; the state is read
    group_sum<THREADS, 1>(votes, s_part);

    Result r = {true, 0, 0, qnan, 0.0};
    if (seeded) r = iterate<THREADS>(s_ax, s_ay, s_part, N, a.set, centre, px, py, valid, m);
    // corr / flow_residual against the keyframe that was matched
    write_corr<THREADS>(s_ax, s_ay, b, N, a.set, centre, px, py, valid, m, r.failed, a.corr, a.flow_residual);

    // the policy: the same decision in every thread
    double x_new = x_old, y_new = y_old, phi_new = phi_old;
    bool replace;
    int new_age, new_misses;
    if (!seeded) {
        replace = true;
        new_age = 0;
        new_misses = 0;
    } else if (!r.failed) {
        double sk, ck;
        sincos(kphi, &sk, &ck);
        phi_new = kphi + m.th;
        x_new = kx + (ck * m.ux - sk * m.uy);
        y_new = ky + (sk * m.ux + ck * m.uy);
        replace = fabs(m.th) > a.key_rot || m.ux * m.ux + m.uy * m.uy > a.key_dist2 ||
            (double)r.matched < a.min_share * votes[0];
        new_age = replace ? 0 : age + 1;
        new_misses = 0;
    } else {
        replace = misses + 1 > a.max_misses;
        new_age = replace ? 0 : age + 1;
        new_misses = replace ? 0 : misses + 1;
    }
    if (replace) {
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            const int i = tid + THREADS * c;
            if (i < N) a.key_ranges[row + i] = valid[c] ? a.in.ranges_cur[row + i] : qnanf;
        }
    }
    if (tid == 0) {
        const bool good = seeded && !r.failed;
        a.motion[3 * b] = good ? m.th : qnan;
        a.motion[3 * b + 1] = good ? m.ux : qnan;
        a.motion[3 * b + 2] = good ? m.uy : qnan;
        a.count[b] = r.matched;
        a.rms[b] = good ? r.rms : qnan;
        a.ok[b] = good ? 1 : 0;
        a.iters_used[b] = r.used;
        a.obs[b] = r.obs;
        a.key_replaced[b] = replace ? 1 : 0;
        a.pose[3 * b] = x_new;
        a.pose[3 * b + 1] = y_new;
        a.pose[3 * b + 2] = phi_new;
        if (replace) {
            a.key_pose[3 * b] = x_new;
            a.key_pose[3 * b + 1] = y_new;
            a.key_pose[3 * b + 2] = phi_new;
            a.key_rel[3 * b] = a.key_rel[3 * b + 1] = a.key_rel[3 * b + 2] = 0.0;
        } else if (good) {
            a.key_rel[3 * b] = m.th;
            a.key_rel[3 * b + 1] = m.ux;
            a.key_rel[3 * b + 2] = m.uy;
        }
        a.key_valid[b] = 1;
        a.key_age[b] = new_age;
        a.key_misses[b] = new_misses;
        if (a.rot) {
            double s1, c1;
            sincos(phi_new, &s1, &c1);
            a.rot[4 * b] = (float)c1;
            a.rot[4 * b + 1] = (float)(-s1);
            a.rot[4 * b + 2] = (float)s1;
            a.rot[4 * b + 3] = (float)c1;
        }
        if (a.trans) {
            a.trans[2 * b] = x_new;
            a.trans[2 * b + 1] = y_new;
        }
        if (a.flow_trans) {
            a.flow_trans[2 * b] = good ? x_new - x_old : 0.0;
            a.flow_trans[2 * b + 1] = good ? y_new - y_old : 0.0;
        }
    }
}

}  // namespace

extern "C" int pof_keyframe_match(const float *ranges_cur, const double *tab, const int32_t *instance_mask,
                                  const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range,
                                  int window, double gate, double max_gap, double huber_delta, int iters,
                                  double eps_theta, double eps_u, double min_pivot, double key_dist, double key_rot,
                                  double min_share, int max_misses, int B, int N, float *key_ranges, double *key_pose,
                                  double *key_rel, uint8_t *key_valid, int32_t *key_age, int32_t *key_misses,
                                  double *pose, double *motion, int32_t *count, double *rms, uint8_t *ok,
                                  int32_t *iters_used, double *obs, uint8_t *key_replaced, int32_t *corr,
                                  double *flow_residual, float *rot, double *trans, double *flow_trans,
                                  pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges_cur || !tab || !key_ranges || !key_pose || !key_rel || !key_valid || !key_age || !key_misses || !pose)
        return POF_E_BADARG;
    if (!motion || !count || !rms || !ok || !iters_used || !obs || !key_replaced) return POF_E_BADARG;
    if (check_settings(window, gate, max_gap, huber_delta, iters, instance_mask, num_det, det_cls, B, N) != POF_OK)
        return POF_E_BADARG;
    if (!(key_dist >= 0.0) || !(key_rot >= 0.0) || !(min_share >= 0.0) || max_misses < 0) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_scan_match and the NMS
    if (B == 0) return POF_OK;
    KeyframeArgs a;
    a.in = {ranges_cur, tab, instance_mask, num_det, det_cls, cls_thresh, max_range};
    a.set = {gate * gate, max_gap * max_gap, huber_delta, eps_theta, eps_u, min_pivot, window, iters};
    a.key_rot = key_rot; a.key_dist2 = key_dist * key_dist; a.min_share = min_share; a.max_misses = max_misses; a.N = N;
    a.key_ranges = key_ranges; a.key_pose = key_pose; a.key_rel = key_rel; a.key_valid = key_valid;
    a.key_age = key_age; a.key_misses = key_misses; a.pose = pose;
    a.motion = motion; a.count = count; a.rms = rms; a.ok = ok; a.iters_used = iters_used; a.obs = obs;
    a.key_replaced = key_replaced; a.corr = corr; a.flow_residual = flow_residual; a.rot = rot; a.trans = trans;
    a.flow_trans = flow_trans;
    if (N <= kWaveMaxN)
        keyframe_match_kernel<64><<<B, 64, 0, pof_stream(stream)>>>(a);
    else
        keyframe_match_kernel<kGroupThreads><<<B, kGroupThreads, 0, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
