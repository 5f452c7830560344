// N9 and N10: keyframe scan matching -- the current scan is matched against a reference scan (the keyframe) that stays
// fixed until the sensor has moved away from it, and the pose is key_pose o (theta, u): no fit error accumulates while
// one keyframe is held.  pof_keyframe_match (N9) keeps one keyframe per sensor; pof_keyframe_map_match (N10) keeps a
// ring of `keys`, matches against the ACTIVE one, and when the sensor leaves it first looks for a stored keyframe it
// has come back to and switches to that one; only without one it stores a new keyframe (into a free slot, else over
// the least recently active one).  The next match against a revisited keyframe forms the pose from that keyframe's
// stored pose, so everything accumulated since it was stored is dropped.
//
// Both entry points run ONE kernel template: what only the ring needs lives in `Ring` and every statement that uses
// it stands inside `if constexpr (RingT::on)`.  N9 instantiates the kernel with `NoRing`, which has none of those
// members -- a ring-only statement outside a guard does not compile -- so K is the constant 1 and the active slot the
// constant 0: no slot search, no second barrier, no store to a ring-only array.  With keys = 1 N10 leaves N9's bits.
// One launch per batch, one sensor per workgroup; all state is persistent and updated in place, so a captured step
// stays one linear chain with no host decision.  The reference has no scan matcher: the specification is the N9 and
// N10 comments of include/pof_abi.h, restated in float64 NumPy by tests/test_keyframe.py (keyframe_oracle) and
// tests/test_keyframe_map.py (keyframe_map_oracle).  This file states only what differs from pof_scan_match
// (scan_match.hip): everything from the gate to the stop rule is the one copy in pof_icp.h.
//
// Window centre.  The keyframe may be tens of beams away from the current scan in every direction, so the window of a
// point is centred on the beam its transformed position falls on:
//   q = R(theta) p + u,  mid = (int)clamp(rint((atan2(q_y, q_x) - tab[0]) / dphi), -N, 2N)
// (0 when dphi == 0, -N for a NaN), searched over [mid - W, mid + W] n [0, N) upwards with a strict <.  No wrap-around.
//
// Hazards.  A workgroup touches the rows of its own sensor only.
//   * Reads before the first barrier: the row of the active slot is read only while staging, and the scalar state of
//     the sensor and of the active slot is read by every thread, all before the first barrier.
//   * Own-beam stores: a row is written after the last correspondence pass, every thread the beams it staged itself
//     -- the replacement is in place when the written slot is the active one, and no hazard at all when it is another.
//   * The barrier before thread 0's stores, ring only: the slot search reads key_valid / key_pose / key_stamp of the
//     other slots in every thread, in ascending k, so every thread takes the same decision without an atomic; thread 0
//     writes the scalar state only after one more barrier that all threads reach once their search is over.  Without
//     a ring nothing that thread 0 writes is read after the first barrier.
// pof_icp.h is used as it is: `stage` adds b * N to the reference pointer, so it is handed
// key_ranges + ((b * keys + a) - b) * N, a pointer inside the allocation (key_ranges itself without a ring).
//
// As scan_match.hip: the keyframe's vertices staged once in LDS, the current points in registers, every sum in a FIXED
// ORDER (pof_icp.h) plus one, before the loop, that counts the current points that vote.
// N <= 512: one wave per sensor;  N <= 4096: 512 threads per sensor.
#include "pof_icp.h"

namespace {

using namespace pof_icp;

constexpr int kMaxKeys = 64;

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

// what only N10 has; key_ranges, key_pose and key_valid of KeyframeArgs then hold K slots per sensor
struct Ring {
    static constexpr bool on = true;
    int K;
    double rev_rot, rev_dist2;
    int32_t *key_stamp, *key_active, *step;
    uint8_t *key_switched;
    int32_t *key_slot;
};

struct NoRing {
    static constexpr bool on = false;
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

template <int THREADS, class RingT>
__global__ __launch_bounds__(THREADS) void keyframe_kernel(KeyframeArgs a, RingT g)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ double s_ax[kMaxN], s_ay[kMaxN];
    __shared__ double s_part[kSums * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const double qnan = __builtin_nan("");
    const float qnanf = __builtin_nanf("");

    // the sensor's state, the same values in every thread; an active slot outside the ring is read as the nearest one
    int K = 1, act = 0;
    if constexpr (RingT::on) {
        K = g.K;
        act = g.key_active[b];
        act = act < 0 ? 0 : (act >= K ? K - 1 : act);
    }
    const long long ring = (long long)b * K;                   // the sensor's first slot
    double px[kSlots], py[kSlots];
    bool valid[kSlots];
    double votes[1] = {stage<THREADS>(a.in, a.key_ranges + (ring + act - b) * N, b, N, s_ax, s_ay, px, py, valid)};
    const double phi0 = a.in.tab[0];
    BeamCentre centre = {phi0, N > 1 ? a.in.tab[1] - phi0 : 0.0, N};
    const bool seeded = a.key_valid[ring + act] != 0;
    const double x_old = a.pose[3 * b], y_old = a.pose[3 * b + 1], phi_old = a.pose[3 * b + 2];
    const double kx = a.key_pose[3 * (ring + act)], ky = a.key_pose[3 * (ring + act) + 1],
                 kphi = a.key_pose[3 * (ring + act) + 2];
    const int age = a.key_age[b], misses = a.key_misses[b];
    int step = 0;
    if constexpr (RingT::on) step = g.step[b];
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
    bool store = false, switched = false;                      // store: the gated scan goes to `slot` at the new pose
    int slot = act, new_age, new_misses;
    double rel_th = 0.0, rel_x = 0.0, rel_y = 0.0;             // key_rel after a switch
    if (!seeded) {
        store = true;
        new_age = 0;
        new_misses = 0;
    } else if (!r.failed) {
        double sk, ck;
        sincos(kphi, &sk, &ck);
        phi_new = kphi + m.th;
        x_new = kx + (ck * m.ux - sk * m.uy);
        y_new = ky + (sk * m.ux + ck * m.uy);
        const bool left = fabs(m.th) > a.key_rot || m.ux * m.ux + m.uy * m.uy > a.key_dist2;
        const bool stale = (double)r.matched < a.min_share * votes[0];
        new_age = (left || stale) ? 0 : age + 1;
        new_misses = 0;
        store = left || stale;                                 // the sensor has left, or the place has changed
        if constexpr (RingT::on) {
            if (left) {
                // a stored keyframe the sensor has come back to: the nearest that qualifies, ties to the lower k
                int win = -1, free_slot = -1, lru = -1, lru_stamp = 0;
                double win_d2 = 0.0;
                for (int k = 0; k < K; ++k) {
                    if (!a.key_valid[ring + k]) {
                        if (free_slot < 0) free_slot = k;
                        continue;
                    }
                    if (k == act) continue;
                    const int stamp = g.key_stamp[ring + k];
                    if (lru < 0 || stamp < lru_stamp) {
                        lru = k;
                        lru_stamp = stamp;
                    }
                    const double xk = a.key_pose[3 * (ring + k)], yk = a.key_pose[3 * (ring + k) + 1],
                                 pk = a.key_pose[3 * (ring + k) + 2];
                    const double th = remainder(phi_new - pk, 2.0 * M_PI);
                    const double dx = x_new - xk, dy = y_new - yk;
                    double s1, c1;
                    sincos(pk, &s1, &c1);
                    const double ux = c1 * dx + s1 * dy, uy = (-s1) * dx + c1 * dy;
                    const double d2 = ux * ux + uy * uy;
                    if (fabs(th) <= g.rev_rot && d2 <= g.rev_dist2 && (win < 0 || d2 < win_d2)) {
                        win = k;
                        win_d2 = d2;
                        rel_th = th;
                        rel_x = ux;
                        rel_y = uy;
                    }
                }
                if (win >= 0) {
                    store = false;
                    switched = true;
                    slot = win;
                } else {
                    slot = free_slot >= 0 ? free_slot : (lru >= 0 ? lru : act);
                }
            }
        }
    } else {
        store = misses + 1 > a.max_misses;
        new_age = store ? 0 : age + 1;
        new_misses = store ? 0 : misses + 1;
    }
    if (store) {
        float *dst = a.key_ranges + (ring + slot) * N;
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            const int i = tid + THREADS * c;
            if (i < N) dst[i] = valid[c] ? a.in.ranges_cur[row + i] : qnanf;
        }
    }
    if constexpr (RingT::on) __syncthreads();                  // every thread has finished its slot search
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
        a.key_replaced[b] = store ? 1 : 0;
        a.pose[3 * b] = x_new;
        a.pose[3 * b + 1] = y_new;
        a.pose[3 * b + 2] = phi_new;
        if (store) {
            a.key_pose[3 * (ring + slot)] = x_new;
            a.key_pose[3 * (ring + slot) + 1] = y_new;
            a.key_pose[3 * (ring + slot) + 2] = phi_new;
            a.key_rel[3 * b] = a.key_rel[3 * b + 1] = a.key_rel[3 * b + 2] = 0.0;
        } else if (switched) {
            a.key_rel[3 * b] = rel_th;
            a.key_rel[3 * b + 1] = rel_x;
            a.key_rel[3 * b + 2] = rel_y;
        } else if (good) {
            a.key_rel[3 * b] = m.th;
            a.key_rel[3 * b + 1] = m.ux;
            a.key_rel[3 * b + 2] = m.uy;
        }
        if constexpr (RingT::on) {
            if (store) a.key_valid[ring + slot] = 1;           // the ring marks a slot only when it stores
            g.key_switched[b] = switched ? 1 : 0;
            g.key_slot[b] = slot;
            g.key_active[b] = slot;
            g.key_stamp[ring + slot] = step;
            g.step[b] = step + 1;
        } else {
            a.key_valid[b] = 1;                                // the single keyframe: on every step
        }
        a.key_age[b] = new_age;
        a.key_misses[b] = new_misses;
        pof_write_pose_terms(b, x_new, y_new, phi_new, good ? x_new - x_old : 0.0, good ? y_new - y_old : 0.0, a.rot,
                             a.trans, a.flow_trans);
    }
}

// The checks both entry points make after those of their own pointers, and the argument fields they share
// -> POF_OK or POF_E_BADARG.
int keyframe_args(KeyframeArgs &a, const float *ranges_cur, const double *tab, const int32_t *instance_mask,
                  const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range, int window,
                  double gate, double max_gap, double huber_delta, int iters, double eps_theta, double eps_u,
                  double min_pivot, double key_dist, double key_rot, double min_share, int max_misses, int B, int N,
                  float *key_ranges, double *key_pose, double *key_rel, uint8_t *key_valid, int32_t *key_age,
                  int32_t *key_misses, double *pose, double *motion, int32_t *count, double *rms, uint8_t *ok,
                  int32_t *iters_used, double *obs, uint8_t *key_replaced, int32_t *corr, double *flow_residual,
                  float *rot, double *trans, double *flow_trans)
{
    if (check_settings(window, gate, max_gap, huber_delta, iters, instance_mask, num_det, det_cls, B, N) != POF_OK)
        return POF_E_BADARG;
    if (!(key_dist >= 0.0) || !(key_rot >= 0.0) || !(min_share >= 0.0) || max_misses < 0) return POF_E_BADARG;
    a.in = {ranges_cur, tab, {instance_mask, num_det, det_cls, cls_thresh}, max_range};
    a.set = {gate * gate, max_gap * max_gap, huber_delta, eps_theta, eps_u, min_pivot, window, iters};
    a.key_rot = key_rot; a.key_dist2 = key_dist * key_dist; a.min_share = min_share; a.max_misses = max_misses; a.N = N;
    a.key_ranges = key_ranges; a.key_pose = key_pose; a.key_rel = key_rel; a.key_valid = key_valid;
    a.key_age = key_age; a.key_misses = key_misses; a.pose = pose;
    a.motion = motion; a.count = count; a.rms = rms; a.ok = ok; a.iters_used = iters_used; a.obs = obs;
    a.key_replaced = key_replaced; a.corr = corr; a.flow_residual = flow_residual; a.rot = rot; a.trans = trans;
    a.flow_trans = flow_trans;
    return POF_OK;
}

// the size check, which comes after every argument check, and the launch
template <class RingT>
int keyframe_launch(const KeyframeArgs &a, const RingT &g, int B, pof_stream_t stream)
{
    if (a.N > kGroupMaxN) return POF_E_SHAPE;                  // the limit of pof_scan_match and the NMS
    if (B == 0) return POF_OK;
    POF_LAUNCH_PER_SENSOR(keyframe_kernel, a.N, B, stream, a, g);
    POF_CHECK_LAUNCH();
    return POF_OK;
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
    KeyframeArgs a;
    if (keyframe_args(a, ranges_cur, tab, instance_mask, num_det, det_cls, cls_thresh, max_range, window, gate, max_gap,
                      huber_delta, iters, eps_theta, eps_u, min_pivot, key_dist, key_rot, min_share, max_misses, B, N,
                      key_ranges, key_pose, key_rel, key_valid, key_age, key_misses, pose, motion, count, rms, ok,
                      iters_used, obs, key_replaced, corr, flow_residual, rot, trans, flow_trans) != POF_OK)
        return POF_E_BADARG;
    return keyframe_launch(a, NoRing{}, B, stream);
}

extern "C" int pof_keyframe_map_match(const float *ranges_cur, const double *tab, const int32_t *instance_mask,
                                      const int32_t *num_det, const double *det_cls, double cls_thresh,
                                      double max_range, int window, double gate, double max_gap, double huber_delta,
                                      int iters, double eps_theta, double eps_u, double min_pivot, double key_dist,
                                      double key_rot, double min_share, int max_misses, double revisit, int B, int N,
                                      int keys, float *key_ranges, double *key_pose, uint8_t *key_valid,
                                      int32_t *key_stamp, int32_t *key_active, double *key_rel, int32_t *key_age,
                                      int32_t *key_misses, int32_t *step, double *pose, double *motion, int32_t *count,
                                      double *rms, uint8_t *ok, int32_t *iters_used, double *obs, uint8_t *key_replaced,
                                      uint8_t *key_switched, int32_t *key_slot, int32_t *corr, double *flow_residual,
                                      float *rot, double *trans, double *flow_trans, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges_cur || !tab || !key_ranges || !key_pose || !key_valid || !key_stamp || !key_active || !key_rel ||
        !key_age || !key_misses || !step || !pose)
        return POF_E_BADARG;
    if (!motion || !count || !rms || !ok || !iters_used || !obs || !key_replaced || !key_switched || !key_slot)
        return POF_E_BADARG;
    KeyframeArgs a;
    if (keyframe_args(a, ranges_cur, tab, instance_mask, num_det, det_cls, cls_thresh, max_range, window, gate, max_gap,
                      huber_delta, iters, eps_theta, eps_u, min_pivot, key_dist, key_rot, min_share, max_misses, B, N,
                      key_ranges, key_pose, key_rel, key_valid, key_age, key_misses, pose, motion, count, rms, ok,
                      iters_used, obs, key_replaced, corr, flow_residual, rot, trans, flow_trans) != POF_OK)
        return POF_E_BADARG;
    if (keys < 1 || keys > kMaxKeys || !(revisit >= 0.0 && revisit <= 1.0)) return POF_E_BADARG;
    const Ring g = {keys, revisit * key_rot, (revisit * key_dist) * (revisit * key_dist), key_stamp, key_active, step,
                    key_switched, key_slot};
    return keyframe_launch(a, g, B, stream);
}
