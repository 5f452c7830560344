// N17: novelty segments, the NOVEL points of a scan (pof_grid_cast's point_class) grouped into detections in the layout
// of pof_nms_predicted_center.  One launch per batch, one workgroup per sensor, no state; include/pof_abi.h has the
// contract.
//   1. points: p = r (cos, sin) in float64 from tab, one rounding per product; beam i is a member when its class byte is
//      2 (NOVEL) and r is finite and > 0.  All points and the member flags stand whole in LDS.
//   2. break flags: a member looks back over at most max_skip + 1 beams for the nearest member l; it continues l's
//      segment when d2 = dx dx + dy dy <= jump^2, else it starts one.  Thread t does this for the beams 8 t .. 8 t + 7,
//      so a workgroup prefix sum of the starts per thread (group_exclusive) numbers the segments in beam order.
//   3. per segment in LDS: the first beam (its starter alone writes it), the last beam (integer atomicMax), the members
//      that belong to a confident NMS detection (integer atomicAdd); every member's slot now holds its segment + 1.
//   4. sums: pof_sensor::row_sums over the whole staged scan with the segments as rows -- segment s belongs to thread
//      s % THREADS, slot s / THREADS, which alone adds its members' p in ascending beam index and counts them.
//   5. filters by the owner, few before wide; a second prefix sum over the keep flags, slot by slot (segment order is
//      slot-major), gives the row; the owner stores its row's fields, every thread zero-fills the rows at and beyond
//      num_det and turns the segment of its beams into the instance id.
// Integer LDS atomics only (max and counts have no order), no global atomics, plain float64 multiplies and adds
// (-ffp-contract=off), no libm call, one division per kept row: the same bits in every run, at every batch position and
// in a graph replay.
//   N <= 512:  one wave per sensor (THREADS = 64), wave-level ordering only, 18 KiB of LDS;
//   N <= 4096: 512 threads per sensor, workgroup barriers, 144 KiB of LDS whatever the number of segments.
// Latency bound like person_motion.hip, whose point walk it shares; it has no pairwise search behind the walk.
#include <cmath>

#include "pof_sensor.h"

namespace {

using namespace pof_sensor;

constexpr int kClsNovel = 2;                    // pof_grid_cast's point_class NOVEL

struct NovelArgs {
    const float *ranges;
    const double *tab;
    const uint8_t *point_class;
    NmsGate gate;
    double jump2, width2;
    int max_skip, min_points, N;
    int32_t *instance_mask, *num_det;
    double *det_xy, *det_cls;
    int32_t *det_count, *det_first, *det_last;
    double *det_width2;
    int32_t *det_known, *seg_count;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void novel_segments_kernel(NovelArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ double s_p[2][kMaxN];        // the points of the scan
    __shared__ int s_seg[kMaxN];            // per beam: first the member flag, then segment + 1 (0: no member)
    __shared__ int s_first[kMaxN], s_last[kMaxN], s_known[kMaxN];   // per segment
    __shared__ int s_row[kMaxN];            // segment -> row, or -1
    __shared__ int s_part[THREADS / 64], s_drop[2];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const int nms = a.gate.num(b, N);

    // 1. the points and who is a member
    for (int i = tid; i < N; i += THREADS) {
        const double r = (double)a.ranges[row + i];
        s_p[0][i] = r * a.tab[N + 2 * i];
        s_p[1][i] = r * a.tab[N + 2 * i + 1];
        s_seg[i] = a.point_class[row + i] == kClsNovel && isfinite(r) && r > 0.0 ? 1 : 0;
        s_last[i] = -1;
        s_known[i] = 0;
    }
    if (tid < 2) s_drop[tid] = 0;
    pof_lds_order<THREADS>();

    // 2. the members among the beams 8 tid .. 8 tid + 7 and which of them start a segment
    const int i0 = tid * kSlots;
    unsigned member = 0, starts = 0;
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = i0 + c;
        if (i >= N || !s_seg[i]) continue;
        member |= 1u << c;
        int l = -1;
        for (int j = i - 1; j >= 0 && i - j <= a.max_skip + 1; --j) {
            if (s_seg[j]) {
                l = j;
                break;
            }
        }
        bool goes_on = false;
        if (l >= 0) {
            const double dx = s_p[0][i] - s_p[0][l], dy = s_p[1][i] - s_p[1][l];
            goes_on = dx * dx + dy * dy <= a.jump2;
        }
        if (!goes_on) starts |= 1u << c;
    }
    int segs;
    int seg = group_exclusive<THREADS>(__popc(starts), s_part, segs) - 1;   // the segment open in front of beam i0
    segs = __builtin_amdgcn_readfirstlane(segs);
    pof_lds_order<THREADS>();                                  // every member flag is read: the slots change meaning

    // 3. per segment the first and last beam and the members the NMS knows as a person
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = i0 + c;
        if (!(member >> c & 1)) continue;
        if (starts >> c & 1) s_first[++seg] = i;
        s_seg[i] = seg + 1;
        atomicMax(&s_last[seg], i);
        if (a.gate.is_person(row, i, nms)) atomicAdd(&s_known[seg], 1);
    }
    pof_lds_order<THREADS>();

    // 4. the sums of the members' points per segment, in beam order; segment tid + THREADS c is slot c of this thread
    double acc[kSlots][2];
    int cnt[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        cnt[c] = 0;
        acc[c][0] = acc[c][1] = 0.0;
    }
    row_sums<THREADS>(s_seg, s_p, N, segs, acc, cnt);

    // 5. the filters, few before wide, and the rows of the kept segments in segment order
    const int seg_slots = (segs + THREADS - 1) / THREADS;
    double w2[kSlots];
    int first[kSlots], last[kSlots], known[kSlots], out_row[kSlots];
    int rows = 0;
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        out_row[c] = -1;
        if (c < seg_slots) {                                   // wave-uniform
            keep_branch();
            const int s = tid + THREADS * c;
            bool keep = false;
            if (s < segs) {
                first[c] = s_first[s], last[c] = s_last[s], known[c] = s_known[s];
                const double dx = s_p[0][last[c]] - s_p[0][first[c]], dy = s_p[1][last[c]] - s_p[1][first[c]];
                w2[c] = dx * dx + dy * dy;
                if (cnt[c] < a.min_points) atomicAdd(&s_drop[0], 1);
                else if (!(w2[c] <= a.width2)) atomicAdd(&s_drop[1], 1);       // a NaN drops the segment
                else keep = true;
            }
            int kept;
            const int at = rows + group_exclusive<THREADS>(keep ? 1 : 0, s_part, kept);
            rows += kept;
            if (keep) out_row[c] = at;
            if (s < segs) s_row[s] = out_row[c];
        }
    }
    rows = __builtin_amdgcn_readfirstlane(rows);
    pof_lds_order<THREADS>();

#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        if (c < seg_slots) {
            keep_branch();
            if (out_row[c] >= 0) {
                const long long q = row + out_row[c];
                const double m = (double)cnt[c];
                a.det_xy[2 * q] = acc[c][0] / m;
                a.det_xy[2 * q + 1] = acc[c][1] / m;
                a.det_cls[q] = 1.0;
                a.det_count[q] = cnt[c];
                a.det_first[q] = first[c];
                a.det_last[q] = last[c];
                a.det_width2[q] = w2[c];
                a.det_known[q] = known[c];
            }
        }
    }
    for (int i = tid; i < N; i += THREADS) {
        const long long q = row + i;
        const int id = s_seg[i];
        a.instance_mask[q] = id ? s_row[id - 1] + 1 : 0;
        if (i >= rows) {
            a.det_xy[2 * q] = a.det_xy[2 * q + 1] = a.det_cls[q] = a.det_width2[q] = 0.0;
            a.det_count[q] = a.det_first[q] = a.det_last[q] = a.det_known[q] = 0;
        }
    }
    if (tid == 0) {
        a.num_det[b] = rows;
        a.seg_count[3 * (long long)b] = segs;
        a.seg_count[3 * (long long)b + 1] = s_drop[0];
        a.seg_count[3 * (long long)b + 2] = s_drop[1];
    }
}

}  // namespace

extern "C" int pof_novel_segments(const float *ranges, const double *tab, const uint8_t *point_class,
                                  const int32_t *nms_instance_mask, const int32_t *nms_num_det,
                                  const double *nms_det_cls, double cls_thresh, double jump, int max_skip,
                                  int min_points, double max_width, int B, int N, int32_t *instance_mask,
                                  int32_t *num_det, double *det_xy, double *det_cls, int32_t *det_count,
                                  int32_t *det_first, int32_t *det_last, double *det_width2, int32_t *det_known,
                                  int32_t *seg_count, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges || !tab || !point_class || !instance_mask || !num_det || !det_xy || !det_cls || !det_count ||
        !det_first || !det_last || !det_width2 || !det_known || !seg_count)
        return POF_E_BADARG;
    if (!nms_gate_ok(nms_instance_mask, nms_num_det, nms_det_cls)) return POF_E_BADARG;
    if (!(jump > 0.0) || !(max_width >= 0.0) || min_points < 1 || max_skip < 0 || max_skip > 64 || B < 0 || N < 1)
        return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    NovelArgs a;
    a.ranges = ranges; a.tab = tab; a.point_class = point_class;
    a.gate = {nms_instance_mask, nms_num_det, nms_det_cls, cls_thresh};
    a.jump2 = jump * jump; a.width2 = max_width * max_width; a.max_skip = max_skip; a.min_points = min_points; a.N = N;
    a.instance_mask = instance_mask; a.num_det = num_det; a.det_xy = det_xy; a.det_cls = det_cls;
    a.det_count = det_count; a.det_first = det_first; a.det_last = det_last; a.det_width2 = det_width2;
    a.det_known = det_known; a.seg_count = seg_count;
    POF_LAUNCH_PER_SENSOR(novel_segments_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
