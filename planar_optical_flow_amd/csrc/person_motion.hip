// N11: person motion without a flow net, one launch per batch, one workgroup per sensor.
//
// Per detection k < num_det[b] (instance id k + 1) the launch takes the centroid of the detection's own scan points in
// the world frame, pairs it with a centroid of the previous scan by a strict mutual-nearest rule and writes the
// difference as det_flow: the person's displacement per scan, in the shape and meaning of pof_person_flow's det_flow,
// so pof_track_update consumes it unchanged.  include/pof_abi.h has the contract.
//   1. points: p = r (cos, sin) in float64 from tab, w = ((double)R00 p_x + (double)R01 p_y) + t_x (likewise y); a point
//      counts for row k when instance_mask = k + 1 and r is finite and < max_range
//   2. det_centre[k] = the sum of its points' w, added in ascending point index (pof_sensor::row_sums, the walk of
//      pof_person_flow), divided by det_count[k]; det_xy_world / det_valid by pof_person_flow's expressions
//   3. candidates: det_valid, det_count >= min_points, a finite centre
//   4. best(k) = the previous candidate j of smallest d2 = dx dx + dy dy, j upwards with a strict <, while d2 <= reach^2;
//      every previous candidate has a best current candidate by the same rule, k upwards; a pair is mutual
//   5. det_flow[k] = det_centre[k] - prev_centre[j], det_prev[k] = j; NaN and -1 without a pair
//   6. after a barrier the state becomes this scan's centres, candidate flags and num_det
//
// Shape: the per-sensor workgroup of pof_sensor.h; thread t owns the rows t, t + THREADS, ... (kSlots of them, in
// registers) of this scan and of the previous one.  The points go through LDS in chunks of kChunk and are summed per row
// by row_sums: every wave steps through the staged points in ascending index, only the owning lane adds.  The centres
// of both scans then stand whole in LDS, a row that is no candidate as NaN -- a NaN distance is never inside the reach,
// so the search needs no flag -- and every thread goes over the other scan's candidate centres in row order for the
// rows it owns.  Both walks take 64 entries at a time from LDS into a wave's registers and step through the set bits of
// a ballot in ascending order, the entry coming out of its lane by v_readlane: wave-uniform, one LDS read per 64
// entries instead of a dependent one per entry.  Only the register slots that can hold a row, ceil(rows / THREADS) of
// the kSlots, take part in the search, and every test on a slot is a scalar branch (keep_branch).  The previous scan's
// best rows go through LDS for the mutual test.  No atomics, plain float64 multiplies and adds in the stated order
// (-ffp-contract=off; the only fma is the one det_xy_world shares with pof_person_flow): the same bits in every run, at
// every batch position and in a graph replay.
//   N <= 512:  one wave per sensor (THREADS = 64), wave-level ordering only;
//   N <= 4096: 512 threads per sensor, workgroup barriers; 149 504 bytes of LDS whatever the number of candidates.
// Latency bound like the launches it follows; the pairwise search is num_det * prev_num / THREADS distances per thread.
#include <cmath>

#include "pof_sensor.h"

namespace {

using namespace pof_sensor;

struct PersonMotionArgs {
    const float *ranges;
    const double *tab;
    const int32_t *instance_mask, *num_det;
    const double *det_xy, *det_cls;
    const float *rot;
    const double *trans;
    double cls_thresh, max_range, reach;
    int min_points, N;
    double *prev_centre;
    uint8_t *prev_cand;
    int32_t *prev_num;
    double *det_xy_world, *det_flow, *det_centre;
    int32_t *det_count;
    uint8_t *det_valid;
    int32_t *det_prev;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void person_motion_kernel(PersonMotionArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    static_assert(kMaxN >= kChunk, "the staged points borrow the previous centres' rows");
    __shared__ double s_cur[2][kMaxN];      // this scan's centres; NaN = no candidate
    __shared__ double s_prev[2][kMaxN];     // first the staged points' (wx, wy), then the previous scan's centres
    __shared__ int s_id[kChunk];
    __shared__ int s_back[kMaxN];           // previous row -> its best current row, or -1
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const long long row = (long long)b * N;
    const int nd = clamped_num_det(a.num_det, b, N), pn = clamped_num_det(a.prev_num, b, N);   // scalar loop bounds
    // rows t, t + THREADS, ...: only the first ceil(rows / THREADS) register slots of a thread can hold a row
    const int cur_slots = (nd + THREADS - 1) / THREADS, prev_slots = (pn + THREADS - 1) / THREADS;
    const SensorPose pose(a.rot, a.trans, b);
    const double qnan = __builtin_nan(""), inf = __builtin_inf();
    const double reach2 = a.reach * a.reach;

    double acc[kSlots][2];
    int cnt[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        cnt[c] = 0;
        acc[c][0] = acc[c][1] = 0.0;
    }
    // 1., 2. the sums of the points' world positions per row, in point order
    for (int base = 0; base < N; base += kChunk) {
        const int n = N - base < kChunk ? N - base : kChunk;
        for (int j = tid; j < n; j += THREADS) {
            const int i = base + j;
            const double r = (double)a.ranges[row + i];
            pose.point_to_world(r * a.tab[N + 2 * i], r * a.tab[N + 2 * i + 1], s_prev[0][j], s_prev[1][j]);
            s_id[j] = isfinite(r) && r < a.max_range ? a.instance_mask[row + i] : 0;   // 0: left out
        }
        pof_lds_order<THREADS>();
        row_sums<THREADS>(s_id, s_prev, n, nd, acc, cnt);
        pof_lds_order<THREADS>();                              // the next chunk overwrites the staged points
    }

    // 2., 3. the rows this thread owns: of this scan into registers and LDS, of the previous scan into LDS
    double cx[kSlots], cy[kSlots], ox[kSlots], oy[kSlots];
    uint8_t valid[kSlots], cand[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int k = tid + THREADS * c;
        cx[c] = cy[c] = ox[c] = oy[c] = 0.0;
        valid[c] = cand[c] = 0;
        if (k >= N) {
            cnt[c] = 0;
            continue;
        }
        const long long q = row + k;
        if (k < nd) {
            pose.det_to_world(a.det_xy[2 * q], a.det_xy[2 * q + 1], ox[c], oy[c]);
            const double m = (double)cnt[c];                   // 0 / 0 -> NaN, like np.mean of nothing
            cx[c] = acc[c][0] / m;
            cy[c] = acc[c][1] / m;
            valid[c] = a.det_cls[q] >= a.cls_thresh ? 1 : 0;
            cand[c] = valid[c] && cnt[c] >= a.min_points && isfinite(cx[c]) && isfinite(cy[c]) ? 1 : 0;
        } else {
            cnt[c] = 0;
        }
        s_cur[0][k] = cand[c] ? cx[c] : qnan;
        s_cur[1][k] = cand[c] ? cy[c] : qnan;
        const bool was = k < pn && a.prev_cand[q] != 0;
        s_prev[0][k] = was ? a.prev_centre[2 * q] : qnan;
        s_prev[1][k] = was ? a.prev_centre[2 * q + 1] : qnan;
    }
    pof_lds_order<THREADS>();

    // 4. the best previous row of every row this thread owns: j upwards, strict <
    double bd[kSlots];
    int bj[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        bd[c] = inf;
        bj[c] = -1;
    }
    {
        double sx[kSlots], sy[kSlots];                         // cx / cy keep the true centre of a row that is none
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            sx[c] = cand[c] ? cx[c] : qnan;
            sy[c] = cand[c] ? cy[c] : qnan;
        }
        // 64 previous rows at a time in registers, lane l row j0 + l; the candidates among them in ascending l (a row
        // that is none holds a NaN and could never be inside the reach)
        for (int j0 = 0; j0 < pn; j0 += 64) {
            const int mine = j0 + lane;
            const double qx = mine < pn ? s_prev[0][mine] : qnan, qy = mine < pn ? s_prev[1][mine] : qnan;
            unsigned long long todo = __ballot(qx == qx && qy == qy);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1, j = j0 + l;
                todo &= todo - 1;
                const double px = lane_value(qx, l), py = lane_value(qy, l);
#pragma unroll
                for (int c = 0; c < kSlots; ++c) {
                    if (c < cur_slots) {                       // wave-uniform
                        keep_branch();
                        const double dx = sx[c] - px, dy = sy[c] - py;
                        const double d2 = dx * dx + dy * dy;
                        if (d2 <= reach2 && d2 < bd[c]) {
                            bd[c] = d2;
                            bj[c] = j;
                        }
                    }
                }
            }
        }
    }
    // ... and the best current row of every previous row this thread owns: k upwards, the lower k keeps a tie
    {
        double sx[kSlots], sy[kSlots], rd[kSlots];
        int rk[kSlots];
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            const int j = tid + THREADS * c;
            sx[c] = j < N ? s_prev[0][j] : qnan;
            sy[c] = j < N ? s_prev[1][j] : qnan;
            rd[c] = inf;
            rk[c] = -1;
        }
        for (int k0 = 0; k0 < nd; k0 += 64) {
            const int mine = k0 + lane;
            const double qx = mine < nd ? s_cur[0][mine] : qnan, qy = mine < nd ? s_cur[1][mine] : qnan;
            unsigned long long todo = __ballot(qx == qx && qy == qy);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1, k = k0 + l;
                todo &= todo - 1;
                const double zx = lane_value(qx, l), zy = lane_value(qy, l);
#pragma unroll
                for (int c = 0; c < kSlots; ++c) {
                    if (c < prev_slots) {                      // wave-uniform
                        keep_branch();
                        const double dx = zx - sx[c], dy = zy - sy[c];
                        const double d2 = dx * dx + dy * dy;
                        if (d2 <= reach2 && d2 < rd[c]) {
                            rd[c] = d2;
                            rk[c] = k;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            const int j = tid + THREADS * c;
            if (j < N) s_back[j] = rk[c];
        }
    }
    pof_lds_order<THREADS>();

    // 5. the outputs of the rows this thread owns
    double fx[kSlots], fy[kSlots];
    int partner[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int k = tid + THREADS * c;
        fx[c] = fy[c] = 0.0;
        partner[c] = -1;
        if (k >= nd) continue;
        fx[c] = fy[c] = qnan;
        const int j = bj[c];
        if (j >= 0 && s_back[j] == k) {                        // each is the other's best
            fx[c] = cx[c] - s_prev[0][j];
            fy[c] = cy[c] - s_prev[1][j];
            partner[c] = j;
        }
    }
    pof_lds_order<THREADS>();                                  // 6. every read of the state is behind this barrier
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int k = tid + THREADS * c;
        if (k >= N) continue;
        const long long q = row + k;
        a.det_xy_world[2 * q] = ox[c];
        a.det_xy_world[2 * q + 1] = oy[c];
        a.det_flow[2 * q] = fx[c];
        a.det_flow[2 * q + 1] = fy[c];
        a.det_centre[2 * q] = cx[c];
        a.det_centre[2 * q + 1] = cy[c];
        a.det_count[q] = cnt[c];
        a.det_valid[q] = valid[c];
        a.det_prev[q] = partner[c];
        a.prev_centre[2 * q] = cx[c];
        a.prev_centre[2 * q + 1] = cy[c];
        a.prev_cand[q] = cand[c];
    }
    if (tid == 0) a.prev_num[b] = nd;
}

}  // namespace

extern "C" int pof_person_motion(const float *ranges, const double *tab, const int32_t *instance_mask,
                                 const int32_t *num_det, const double *det_xy, const double *det_cls,
                                 const float *rot, const double *trans, double cls_thresh, double max_range,
                                 double reach, int min_points, int B, int N, double *prev_centre, uint8_t *prev_cand,
                                 int32_t *prev_num, double *det_xy_world, double *det_flow, double *det_centre,
                                 int32_t *det_count, uint8_t *det_valid, int32_t *det_prev, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges || !tab || !instance_mask || !num_det || !det_xy || !det_cls || !rot || !trans || !prev_centre ||
        !prev_cand || !prev_num || !det_xy_world || !det_flow || !det_centre || !det_count || !det_valid || !det_prev)
        return POF_E_BADARG;
    if (!(reach >= 0.0) || min_points < 1 || B < 0 || N < 1) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_nms_predicted_center
    if (B == 0) return POF_OK;
    PersonMotionArgs a;
    a.ranges = ranges; a.tab = tab; a.instance_mask = instance_mask; a.num_det = num_det; a.det_xy = det_xy;
    a.det_cls = det_cls; a.rot = rot; a.trans = trans; a.cls_thresh = cls_thresh; a.max_range = max_range;
    a.reach = reach; a.min_points = min_points; a.N = N; a.prev_centre = prev_centre; a.prev_cand = prev_cand;
    a.prev_num = prev_num; a.det_xy_world = det_xy_world; a.det_flow = det_flow; a.det_centre = det_centre;
    a.det_count = det_count; a.det_valid = det_valid; a.det_prev = det_prev;
    POF_LAUNCH_PER_SENSOR(person_motion_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
