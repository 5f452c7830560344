// N18: merged detections, two detection records in the layout of pof_nms_predicted_center -- A, the primary (the NMS's),
// and B, the secondary (the novelty segments') -- made one.  One launch per batch, one workgroup per sensor, no state;
// include/pof_abi.h has the contract.
//   1. ids: per point its A id (0 unless in [1, nA]) with the confident bit, and its B id (0 unless in [1, nB]), whole
//      in LDS.
//   2. per B row in LDS: its members and its confident members (integer atomicAdd).
//   3. the owner decides: B row k belongs to thread k % THREADS, slot k / THREADS; a workgroup prefix sum over the keep
//      flags, slot by slot (row order is slot-major), ranks the kept rows; rank + nA is the merged row, or -2 at and
//      beyond N.  The owner also notes, per appended row, which B row it came from.
//   4. mask: a member of an appended row that is not confident takes that row's id, every other point keeps A's; the
//      points per merged row are counted in LDS (integer atomicAdd).
//   5. stores, thread t rows and points t, t + THREADS, ...: A's rows, the appended rows through the note of 3., zeros
//      behind them, the mask.
// No floating-point arithmetic but the compare with cls_thresh: det_xy and det_cls move as 64-bit words.  Integer LDS
// atomics only (counts have no order), no global atomics, no libm call: the same bits in every run, at every batch
// position and in a graph replay.
//   N <= 512:  one wave per sensor (THREADS = 64), wave-level ordering only, 14 KiB of LDS;
//   N <= 4096: 512 threads per sensor, workgroup barriers, 112 KiB of LDS whatever the number of rows.
#include "pof_sensor.h"

namespace {

using namespace pof_sensor;

constexpr int kConfident = 1 << 16;             // above every id: N <= 4096

struct MergeArgs {
    const int32_t *b_instance_mask, *b_num_det;
    const unsigned long long *b_det_xy, *b_det_cls, *a_det_xy;
    NmsGate a;
    int absorb_pct, N;
    int32_t *instance_mask, *num_det;
    unsigned long long *det_xy, *det_cls;
    int32_t *det_points;
    uint8_t *det_src;
    int32_t *det_row, *b_row, *b_count, *b_known, *merge_count;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void merge_detections_kernel(MergeArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ int s_a[kMaxN];              // per point: A's id or 0, | kConfident; then the merged id
    __shared__ int s_b[kMaxN];              // per point: B's id or 0
    __shared__ int s_cnt[kMaxN], s_known[kMaxN], s_row[kMaxN];      // per B row
    __shared__ int s_from[kMaxN];           // per appended row, counted from nA: its B row
    __shared__ int s_pts[kMaxN];            // per merged row
    __shared__ int s_part[THREADS / 64];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const int nA = a.a.num(b, N), nB = clamped_num_det(a.b_num_det, b, N);

    // 1. both ids per point
    for (int i = tid; i < N; i += THREADS) {
        const int ia = a.a.id_of(row, i), ib = a.b_instance_mask[row + i];
        s_a[i] = (a.a.row_of(ia, nA) >= 0 ? ia : 0) | (a.a.id_is_person(row, ia, nA) ? kConfident : 0);
        s_b[i] = ib >= 1 && ib <= nB ? ib : 0;
        s_cnt[i] = s_known[i] = s_pts[i] = 0;
    }
    pof_lds_order<THREADS>();

    // 2. members and confident members per B row
    for (int i = tid; i < N; i += THREADS) {
        const int ib = s_b[i];
        if (!ib) continue;
        atomicAdd(&s_cnt[ib - 1], 1);
        if (s_a[i] & kConfident) atomicAdd(&s_known[ib - 1], 1);
    }
    pof_lds_order<THREADS>();

    // 3. absorbed or kept, by the row's owner; the kept rows in row order behind A's, while there is room
    const int b_slots = (nB + THREADS - 1) / THREADS;
    int kept_rows = 0;
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        if (c < b_slots) {                                     // wave-uniform
            keep_branch();
            const int k = tid + THREADS * c;
            bool keep = false;
            if (k < nB) {
                const int cnt = s_cnt[k];
                keep = cnt != 0 && !(100 * s_known[k] >= a.absorb_pct * cnt);
            }
            int kept;
            const int at = nA + kept_rows + group_exclusive<THREADS>(keep ? 1 : 0, s_part, kept);
            kept_rows += kept;
            if (k < nB) s_row[k] = !keep ? -1 : at < N ? at : -2;
            if (keep && at < N) s_from[at - nA] = k;
        }
    }
    kept_rows = __builtin_amdgcn_readfirstlane(kept_rows);
    const int appended = kept_rows < N - nA ? kept_rows : N - nA;
    const int rows = nA + appended;
    pof_lds_order<THREADS>();

    // 4. the merged id per point and the points per merged row
    for (int i = tid; i < N; i += THREADS) {
        const int ia = s_a[i], ib = s_b[i];
        int id = ia & (kConfident - 1);
        if (ib && !(ia & kConfident)) {
            const int r = s_row[ib - 1];
            if (r >= 0) id = r + 1;
        }
        s_a[i] = id;
        if (id) atomicAdd(&s_pts[id - 1], 1);
    }
    pof_lds_order<THREADS>();

    // 5. rows and points
    for (int i = tid; i < N; i += THREADS) {
        const long long q = row + i;
        unsigned long long x = 0, y = 0, cls = 0;
        int src = 0, from = 0;
        if (i < nA) {
            x = a.a_det_xy[2 * q], y = a.a_det_xy[2 * q + 1];
            cls = reinterpret_cast<const unsigned long long *>(a.a.det_cls)[q];
            src = 1, from = i;
        } else if (i < rows) {
            from = s_from[i - nA];
            x = a.b_det_xy[2 * (row + from)], y = a.b_det_xy[2 * (row + from) + 1];
            cls = a.b_det_cls[row + from];
            src = 2;
        }
        a.det_xy[2 * q] = x;
        a.det_xy[2 * q + 1] = y;
        a.det_cls[q] = cls;
        a.det_points[q] = i < rows ? s_pts[i] : 0;
        a.det_src[q] = (uint8_t)src;
        a.det_row[q] = from;
        a.b_row[q] = i < nB ? s_row[i] : -1;
        a.b_count[q] = i < nB ? s_cnt[i] : 0;
        a.b_known[q] = i < nB ? s_known[i] : 0;
        a.instance_mask[q] = s_a[i];
    }
    if (tid == 0) {
        a.num_det[b] = rows;
        int32_t *mc = a.merge_count + 4 * (long long)b;
        mc[0] = nA, mc[1] = appended, mc[2] = nB - kept_rows, mc[3] = kept_rows - appended;
    }
}

}  // namespace

extern "C" int pof_merge_detections(const int32_t *b_instance_mask, const int32_t *b_num_det, const double *b_det_xy,
                                    const double *b_det_cls, const int32_t *a_instance_mask, const int32_t *a_num_det,
                                    const double *a_det_xy, const double *a_det_cls, double cls_thresh, int absorb_pct,
                                    int B, int N, int32_t *instance_mask, int32_t *num_det, double *det_xy,
                                    double *det_cls, int32_t *det_points, uint8_t *det_src, int32_t *det_row,
                                    int32_t *b_row, int32_t *b_count, int32_t *b_known, int32_t *merge_count,
                                    pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!b_instance_mask || !b_num_det || !b_det_xy || !b_det_cls || !instance_mask || !num_det || !det_xy || !det_cls ||
        !det_points || !det_src || !det_row || !b_row || !b_count || !b_known || !merge_count)
        return POF_E_BADARG;
    if (!nms_gate_ok(a_instance_mask, a_num_det, a_det_cls) || (a_det_xy != nullptr) != (a_instance_mask != nullptr))
        return POF_E_BADARG;
    if (absorb_pct < 0 || absorb_pct > 101 || B < 0 || N < 1) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    MergeArgs a;
    a.b_instance_mask = b_instance_mask; a.b_num_det = b_num_det;
    a.b_det_xy = reinterpret_cast<const unsigned long long *>(b_det_xy);
    a.b_det_cls = reinterpret_cast<const unsigned long long *>(b_det_cls);
    a.a_det_xy = reinterpret_cast<const unsigned long long *>(a_det_xy);
    a.a = {a_instance_mask, a_num_det, a_det_cls, cls_thresh};
    a.absorb_pct = absorb_pct; a.N = N;
    a.instance_mask = instance_mask; a.num_det = num_det;
    a.det_xy = reinterpret_cast<unsigned long long *>(det_xy);
    a.det_cls = reinterpret_cast<unsigned long long *>(det_cls);
    a.det_points = det_points; a.det_src = det_src; a.det_row = det_row; a.b_row = b_row; a.b_count = b_count;
    a.b_known = b_known; a.merge_count = merge_count;
    POF_LAUNCH_PER_SENSOR(merge_detections_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
