// N15: map-checked tracks, per-track evidence from the occupancy grid.  One launch per batch in the per-sensor workgroup
// form of pof_sensor.h; include/pof_abi.h has the contract.
//
// The detection row of the NMS is a rank that changes with every scan; only the track slot carries identity.  The
// launch joins what pof_grid_map_update says about the row a track was matched with (det_points, det_free, and how many
// of the row's points lie on cells that were occupied before this scan) to that slot, keeps the sums per slot, and
// derives a class from them and from how far the track has travelled:
//   0. det_occ per row: the beams of the sensor, thread t the beams t, t + THREADS, ..., counted with integer LDS atomics
//      as the points launch of grid_map.hip counts det_points (integer sums have no order)
//   1.-3. per slot, thread t the slots t, t + THREADS, ... (one wave: lane l owns l, l + 64, ...): a freed slot is
//      zeroed, a reused one restarts, a live one adds its row's counts, fades them beyond `cap` and looks whether the track
//      has left the place where its evidence started
//   4. the class, a pure function of the slot's state, in int64 products
//   5. det_class by an integer LDS atomicMin over the slot index (the lower slot stands, whatever the order),
//      point_class through the instance ids, class_count with integer LDS atomics
// The slot count M <= 256 is small beside N: at most four slots per lane in the one-wave form, one per thread in the
// other.  No global atomics, no floating-point atomics, float64 in plain multiplies and adds (-ffp-contract=off): the
// same bits in every run, at every batch position and in a graph replay.  Latency bound like the launches it follows.
#include <climits>

#include "pof_sensor.h"

namespace {

using namespace pof_sensor;

constexpr int kMaxTracks = 256;
constexpr int kMaxCap = 1 << 20;
constexpr int kMaxScans = 1 << 30;

struct TrackMapArgs {
    const int32_t *instance_mask, *num_det, *point_cell;
    const int16_t *point_prior;
    const int32_t *det_points, *det_free, *track_id;
    const double *track_state;
    const int32_t *track_det;
    int N, M;
    int32_t *ev_id, *ev_points, *ev_free, *ev_occ, *ev_scans;
    double *ev_start;
    uint8_t *ev_moved;
    int32_t *det_occ;
    uint8_t *track_class, *det_class, *point_class;
    int32_t *class_count;
    int occ_thresh, free_pct, occ_pct, min_points, min_scans, cap;
    double travel;
};

// a sum of counts in int32 that wraps like the restatement's instead of overflowing
__device__ __forceinline__ int wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

template <int THREADS>
__global__ __launch_bounds__(THREADS) void track_map_kernel(TrackMapArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ int s_occ[kMaxN];                               // det_occ of this sensor
    __shared__ int s_owner[kMaxN];                             // the lowest live slot that names the row, or INT_MAX
    __shared__ uint8_t s_dclass[kMaxN];                        // det_class of this sensor
    __shared__ uint8_t s_class[kMaxTracks];
    __shared__ int s_count[4];
    const int N = a.N, M = a.M, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N, trow = (long long)b * M;
    const int nd = clamped_num_det(a.num_det, b, N);

    for (int k = tid; k < N; k += THREADS) {
        s_occ[k] = 0;
        s_owner[k] = INT_MAX;
    }
    if (tid < 4) s_count[tid] = 0;
    pof_lds_order<THREADS>();

    // 0. per row the points on cells that were occupied before this scan
    for (int i = tid; i < N; i += THREADS) {
        const int id = a.instance_mask[row + i];
        if (id >= 1 && id <= nd && a.point_cell[row + i] >= 0 && (int)a.point_prior[row + i] >= a.occ_thresh)
            atomicAdd(&s_occ[id - 1], 1);
    }
    pof_lds_order<THREADS>();

    const double travel2 = a.travel * a.travel;
    for (int s = tid; s < M; s += THREADS) {
        const long long at = trow + s;
        const int id = a.track_id[at];
        const double x = a.track_state[4 * at], y = a.track_state[4 * at + 1];
        int eid = a.ev_id[at], points = a.ev_points[at], free_ = a.ev_free[at], occ = a.ev_occ[at];
        int scans = a.ev_scans[at], moved = a.ev_moved[at];
        double sx = a.ev_start[2 * at], sy = a.ev_start[2 * at + 1];
        const bool live = id != 0;
        if (!live) {                                           // 1. a free slot holds zeros
            eid = points = free_ = occ = scans = moved = 0;
            sx = sy = 0.0;
        } else if (id != eid) {                                // a reused slot: the evidence starts again, here
            points = free_ = occ = scans = moved = 0;
            eid = id;
            sx = x;
            sy = y;
        }
        int cls = 0;
        if (live) {
            const int k = a.track_det[at];
            if (k >= 0 && k < nd) {
                atomicMin(&s_owner[k], s);
                const int n = a.det_points[row + k];
                if (n > 0) {                                   // 2. this scan's counts of the track's row
                    points = wrap_add(points, n);
                    free_ = wrap_add(free_, a.det_free[row + k]);
                    occ = wrap_add(occ, s_occ[k]);
                    if (scans < kMaxScans) ++scans;
                    if (points > a.cap) {                      // old evidence fades, the ratios stay
                        points >>= 1;
                        free_ >>= 1;
                        occ >>= 1;
                    }
                }
            }
            const double dx = x - sx, dy = y - sy;             // 3. sticky; a NaN compares false
            const double d2 = dx * dx + dy * dy;
            if (d2 >= travel2) moved = 1;
            // 4. background first: a false positive that slides along a wall does travel
            if (scans >= a.min_scans && points >= a.min_points) {
                if (100ll * occ >= (long long)a.occ_pct * points)
                    cls = 3;
                else if (moved || 100ll * free_ >= (long long)a.free_pct * points)
                    cls = 1;
                else
                    cls = 2;
            }
            atomicAdd(&s_count[cls], 1);
        }
        s_class[s] = (uint8_t)cls;
        a.ev_id[at] = eid;
        a.ev_points[at] = points;
        a.ev_free[at] = free_;
        a.ev_occ[at] = occ;
        a.ev_scans[at] = scans;
        a.ev_start[2 * at] = sx;
        a.ev_start[2 * at + 1] = sy;
        a.ev_moved[at] = (uint8_t)moved;
        a.track_class[at] = (uint8_t)cls;
    }
    pof_lds_order<THREADS>();

    // 5. per row, then per point
    for (int k = tid; k < N; k += THREADS) {
        const int owner = s_owner[k];                          // < M where a live slot named the row (then k < nd)
        const uint8_t cls = owner < M ? s_class[owner] : (uint8_t)0;
        s_dclass[k] = cls;
        a.det_class[row + k] = cls;
        a.det_occ[row + k] = k < nd ? s_occ[k] : 0;
    }
    pof_lds_order<THREADS>();
    for (int i = tid; i < N; i += THREADS) {
        const int id = a.instance_mask[row + i];
        a.point_class[row + i] = id >= 1 && id <= nd ? s_dclass[id - 1] : (uint8_t)0;
    }
    if (tid < 4) a.class_count[4 * b + tid] = s_count[tid];
}

}  // namespace

extern "C" int pof_track_map(const int32_t *instance_mask, const int32_t *num_det, const int32_t *point_cell,
                             const int16_t *point_prior, const int32_t *det_points, const int32_t *det_free,
                             const int32_t *track_id, const double *track_state, const int32_t *track_det, int B, int N,
                             int max_tracks, int32_t *ev_id, int32_t *ev_points, int32_t *ev_free, int32_t *ev_occ,
                             int32_t *ev_scans, double *ev_start, uint8_t *ev_moved, int32_t *det_occ,
                             uint8_t *track_class, uint8_t *det_class, uint8_t *point_class, int32_t *class_count,
                             int occ_thresh, int free_pct, int occ_pct, int min_points, int min_scans, double travel,
                             int cap, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!instance_mask || !num_det || !point_cell || !point_prior || !det_points || !det_free || !track_id ||
        !track_state || !track_det || !ev_id || !ev_points || !ev_free || !ev_occ || !ev_scans || !ev_start ||
        !ev_moved || !det_occ || !track_class || !det_class || !point_class || !class_count)
        return POF_E_BADARG;
    if (B < 0 || N < 1 || max_tracks < 1 || occ_thresh < 0 || free_pct < 0 || free_pct > 100 || occ_pct < 0 ||
        occ_pct > 100 || min_points < 0 || min_scans < 0 || cap < N || cap > kMaxCap || !(travel >= 0.0))
        return POF_E_BADARG;
    if (N > kGroupMaxN || max_tracks > kMaxTracks) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    TrackMapArgs a;
    a.instance_mask = instance_mask; a.num_det = num_det; a.point_cell = point_cell; a.point_prior = point_prior;
    a.det_points = det_points; a.det_free = det_free; a.track_id = track_id; a.track_state = track_state;
    a.track_det = track_det; a.N = N; a.M = max_tracks; a.ev_id = ev_id; a.ev_points = ev_points; a.ev_free = ev_free;
    a.ev_occ = ev_occ; a.ev_scans = ev_scans; a.ev_start = ev_start; a.ev_moved = ev_moved; a.det_occ = det_occ;
    a.track_class = track_class; a.det_class = det_class; a.point_class = point_class; a.class_count = class_count;
    a.occ_thresh = occ_thresh; a.free_pct = free_pct; a.occ_pct = occ_pct; a.min_points = min_points;
    a.min_scans = min_scans; a.cap = cap; a.travel = travel;
    POF_LAUNCH_PER_SENSOR(track_map_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
