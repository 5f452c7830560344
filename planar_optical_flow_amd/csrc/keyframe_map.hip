// N10: keyframe map -- pof_keyframe_match (N9, keyframe_match.hip) with a ring of `keys` keyframes per sensor instead
// of one.  The scan is matched against the ACTIVE keyframe exactly as N9 matches against its only one (the same
// pof_icp.h, the same beam-projected window centre); what is new is what happens when the sensor leaves it: it first
// looks for a stored keyframe it has come back to and switches to that one, and only without one stores a new keyframe
// (into a free slot, else over the least recently active one).  The next match against a revisited keyframe forms the
// pose from that keyframe's stored pose, so everything accumulated since it was stored is dropped.  The reference has
// no scan matcher: the specification is the N10 comment of include/pof_abi.h, restated in float64 NumPy by
// tests/test_keyframe_map.py (keyframe_map_oracle).  With keys = 1 every decision below reduces to N9's.
//
// One launch per batch, one sensor per workgroup.  Hazards:
//   * the row of the active slot is read only while staging (before the first barrier); a row is written after the last
//     correspondence pass, every thread the beams it staged itself -- N9's in-place argument when the written slot is
//     the active one, and no hazard at all when it is another;
//   * the scalar state of the active slot is read by every thread before the first barrier; the slot search reads
//     key_valid / key_pose / key_stamp of the other slots in every thread, in ascending k, so every thread takes the
//     same decision without an atomic; thread 0 writes the scalar state only after one more barrier that all threads
//     reach once their search is over.
// A workgroup touches the rows of its own sensor only.  pof_icp.h is used as it is: `stage` adds b * N to the
// reference pointer, so it is handed key_ranges + ((b * keys + a) - b) * N, a pointer inside the allocation.
// N <= 512: one wave per sensor;  N <= 4096: 512 threads per sensor.
#include "pof_icp.h"

namespace {

using namespace pof_icp;

constexpr int kMaxKeys = 64;

struct KeyframeMapArgs {
    Input in;
    Settings set;
    double key_rot, key_dist2, min_share, rev_rot, rev_dist2;
    int max_misses, N, K;
    float *key_ranges;
    double *key_pose;
    uint8_t *key_valid;
    int32_t *key_stamp, *key_active;
    double *key_rel;
    int32_t *key_age, *key_misses, *step;
    double *pose;
    double *motion;
    int32_t *count;
    double *rms;
    uint8_t *ok;
    int32_t *iters_used;
    double *obs;
    uint8_t *key_replaced, *key_switched;
    int32_t *key_slot;
    int32_t *corr;
    double *flow_residual;
    float *rot;
    double *trans, *flow_trans;
};

// N9's window centre (keyframe_match.hip): the beam the transformed point q falls on; phi0 = tab[0]
__device__ __forceinline__ int beam_of(double qx, double qy, double phi0, double dphi, int N)
{
    if (dphi == 0.0) return 0;
    double t = rint((atan2(qy, qx) - phi0) / dphi);
    if (!(t >= (double)-N)) t = (double)-N;
    if (!(t <= (double)(2 * N))) t = (double)(2 * N);
    return (int)t;
}

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
__global__ __launch_bounds__(THREADS) void keyframe_map_kernel(KeyframeMapArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ double s_ax[kMaxN], s_ay[kMaxN];
    __shared__ double s_part[kSums * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, K = a.K, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const long long ring = (long long)b * K;                   // the sensor's first slot
    const double qnan = __builtin_nan("");
    const float qnanf = __builtin_nanf("");

    // the sensor's state, the same values in every thread; an active slot outside the ring is read as the nearest one
    int act = a.key_active[b];
    act = act < 0 ? 0 : (act >= K ? K - 1 : act);
    double px[kSlots], py[kSlots];
    bool valid[kSlots];
    double votes[1] = {stage<THREADS>(a.in, a.key_ranges + (ring + act - b) * N, b, N, s_ax, s_ay, px, py, valid)};
    const double phi0 = a.in.tab[0];
    BeamCentre centre = {phi0, N > 1 ? a.in.tab[1] - phi0 : 0.0, N};
    const bool seeded = a.key_valid[ring + act] != 0;
    const double x_old = a.pose[3 * b], y_old = a.pose[3 * b + 1], phi_old = a.pose[3 * b + 2];
    const double kx = a.key_pose[3 * (ring + act)], ky = a.key_pose[3 * (ring + act) + 1],
                 kphi = a.key_pose[3 * (ring + act) + 2];
    const int age = a.key_age[b], misses = a.key_misses[b], step = a.step[b];
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
                const int stamp = a.key_stamp[ring + k];
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
                if (fabs(th) <= a.rev_rot && d2 <= a.rev_dist2 && (win < 0 || d2 < win_d2)) {
                    win = k;
                    win_d2 = d2;
                    rel_th = th;
                    rel_x = ux;
                    rel_y = uy;
                }
            }
            if (win >= 0) {
                switched = true;
                slot = win;
            } else {
                store = true;
                slot = free_slot >= 0 ? free_slot : (lru >= 0 ? lru : act);
            }
        } else if (stale) {
            store = true;                                      // the place has changed: slot `act` in place
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
    __syncthreads();                                           // every thread has finished its slot search
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
        a.key_switched[b] = switched ? 1 : 0;
        a.key_slot[b] = slot;
        a.pose[3 * b] = x_new;
        a.pose[3 * b + 1] = y_new;
        a.pose[3 * b + 2] = phi_new;
        if (store) {
            a.key_pose[3 * (ring + slot)] = x_new;
            a.key_pose[3 * (ring + slot) + 1] = y_new;
            a.key_pose[3 * (ring + slot) + 2] = phi_new;
            a.key_rel[3 * b] = a.key_rel[3 * b + 1] = a.key_rel[3 * b + 2] = 0.0;
            a.key_valid[ring + slot] = 1;
        } else if (switched) {
            a.key_rel[3 * b] = rel_th;
            a.key_rel[3 * b + 1] = rel_x;
            a.key_rel[3 * b + 2] = rel_y;
        } else if (good) {
            a.key_rel[3 * b] = m.th;
            a.key_rel[3 * b + 1] = m.ux;
            a.key_rel[3 * b + 2] = m.uy;
        }
        a.key_active[b] = slot;
        a.key_stamp[ring + slot] = step;
        a.step[b] = step + 1;
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
    if (check_settings(window, gate, max_gap, huber_delta, iters, instance_mask, num_det, det_cls, B, N) != POF_OK)
        return POF_E_BADARG;
    if (!(key_dist >= 0.0) || !(key_rot >= 0.0) || !(min_share >= 0.0) || max_misses < 0) return POF_E_BADARG;
    if (keys < 1 || keys > kMaxKeys || !(revisit >= 0.0 && revisit <= 1.0)) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_scan_match and the NMS
    if (B == 0) return POF_OK;
    KeyframeMapArgs a;
    a.in = {ranges_cur, tab, instance_mask, num_det, det_cls, cls_thresh, max_range};
    a.set = {gate * gate, max_gap * max_gap, huber_delta, eps_theta, eps_u, min_pivot, window, iters};
    a.key_rot = key_rot; a.key_dist2 = key_dist * key_dist; a.min_share = min_share;
    a.rev_rot = revisit * key_rot; a.rev_dist2 = (revisit * key_dist) * (revisit * key_dist);
    a.max_misses = max_misses; a.N = N; a.K = keys;
    a.key_ranges = key_ranges; a.key_pose = key_pose; a.key_valid = key_valid; a.key_stamp = key_stamp;
    a.key_active = key_active; a.key_rel = key_rel; a.key_age = key_age; a.key_misses = key_misses; a.step = step;
    a.pose = pose;
    a.motion = motion; a.count = count; a.rms = rms; a.ok = ok; a.iters_used = iters_used; a.obs = obs;
    a.key_replaced = key_replaced; a.key_switched = key_switched; a.key_slot = key_slot; a.corr = corr;
    a.flow_residual = flow_residual; a.rot = rot; a.trans = trans; a.flow_trans = flow_trans;
    if (N <= kWaveMaxN)
        keyframe_map_kernel<64><<<B, 64, 0, pof_stream(stream)>>>(a);
    else
        keyframe_map_kernel<kGroupThreads><<<B, kGroupThreads, 0, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
