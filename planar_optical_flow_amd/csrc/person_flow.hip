// N5: per-person flow in the world frame (depracted_scripts/infer_person_flow.py:134-157,
// src/utils/viz_utils.py:556-575 plot_person_flow_fixed_pose), one launch per batch.
//
// Per point i of scan b:
//   1. g  = canonical_to_global_flow_torch(flow_canonical)      float32, pof_rotate_flow_point (== pof_rotate_flow)
//   2. w32[c] = fmaf(g1, Rt[1][c], g0 * Rt[0][c]),  Rt = rot[b]^T   float32: the order in which sgemm evaluates
//      np.matmul(pred_flow, odom_rot.T) for three rows and more;  w[c] = (double)w32[c] + flow_trans[b][c]
//   3. rgb = flow_to_hsv(w) (src/utils/utils.py:574-584): hypot / atan2 as pof_xy_to_rphi, then the arithmetic of
//      colorsys.hsv_to_rgb with value 1; saturation 0 is exactly white.
// Per detection k < num_det[b] (instance id k + 1): the count of its points, the float64 means of w and rgb over
// them, the world centre fma(d1, Rt[1][c], d0 * Rt[0][c]) + trans[b][c] and cls >= cls_thresh.  Rows k >= num_det[b]
// are zeros.  A detection without points (a later kept centre took them all) has count 0 and NaN means, like
// np.mean of an empty selection.
//
// The sums are SEQUENTIAL IN POINT ORDER with plain float64 adds: no atomics, nothing that depends on scheduling, so
// a result is the same bits in every run and in a graph replay.  The per-sensor workgroup of pof_sensor.h: it stages
// (id, wx, wy, r, g, b) of up to kChunk points in LDS; thread t owns the instances t, t + THREADS, ... (kSlots
// accumulators in registers); every wave then walks the staged points in index order and only the owning lane adds
// (pof_sensor::row_sums).  One wave per scan up to N = 512, 512 threads and chunks of 512 points between workgroup
// barriers up to N = 4096, the same point order in both.
// Latency bound like the NMS it follows; reported in microseconds.
#include <cmath>

#include "pof_sensor.h"

namespace {

using namespace pof_sensor;

struct PersonFlowArgs {
    const float *flow_canonical;
    const double *tab;
    const int32_t *instance_mask, *num_det;
    const double *det_xy, *det_cls;
    const float *rot;
    const double *trans, *flow_trans;
    double cls_thresh;
    int N;
    float *flow_global;
    double *flow_world, *rgb, *det_xy_world, *det_flow, *det_rgb;
    int32_t *det_count;
    uint8_t *det_valid;
};

// flow_to_hsv for one vector (the arithmetic of utils.flow_to_hsv / colorsys.hsv_to_rgb, value 1)
__device__ __forceinline__ void flow_colour(double wx, double wy, double &cr, double &cg, double &cb)
{
    const double r = hypot(wx, wy), phi = atan2(wy, wx);
    const double h = (phi + 2.0 * M_PI) / M_PI / 2;
    const double sat = (r > 0.1 ? 0.1 : r) / 0.1;             // np.minimum keeps a NaN
    const double h6 = h * 6.0;
    // int(): truncation; h is in [0.5, 1.5].  A NaN flow has no sector: NumPy's cast gives INT64_MIN, whose
    // remainder by 6 (Python's sign convention) is 4 -- stated here, the C++ cast of a NaN is undefined
    const long long sector = h6 != h6 ? 4 : (long long)h6;
    const double f = h6 - (double)sector;
    const double v = 1.0;
    const double p = v * (1.0 - sat), q = v * (1.0 - sat * f), t = v * (1.0 - sat * (1.0 - f));
    switch ((int)(((sector % 6) + 6) % 6)) {
        case 0: cr = v; cg = t; cb = p; break;
        case 1: cr = q; cg = v; cb = p; break;
        case 2: cr = p; cg = v; cb = t; break;
        case 3: cr = p; cg = q; cb = v; break;
        case 4: cr = t; cg = p; cb = v; break;
        default: cr = v; cg = p; cb = q; break;
    }
    if (sat == 0.0) cr = cg = cb = v;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void person_flow_kernel(PersonFlowArgs a)
{
    __shared__ double s_v[5][kChunk];       // wx, wy, r, g, b of the staged points
    __shared__ int s_id[kChunk];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const int nd = clamped_num_det(a.num_det, b, N);
    const SensorPose pose(a.rot, a.trans, b);                  // Rt[r][c] = rot[b][c][r]
    const float r00 = pose.r00, r01 = pose.r01, r10 = pose.r10, r11 = pose.r11;
    const double ftx = a.flow_trans[2 * b], fty = a.flow_trans[2 * b + 1];

    double acc[kSlots][5];
    int cnt[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        cnt[c] = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[c][j] = 0.0;
    }
    for (int base = 0; base < N; base += kChunk) {
        const int n = N - base < kChunk ? N - base : kChunk;
        for (int j = tid; j < n; j += THREADS) {
            const int i = base + j;
            const long long p = row + i;
            float g0, g1;
            pof_rotate_flow_point<float>(a.tab[N + 2 * i], a.tab[N + 2 * i + 1], a.flow_canonical[2 * p],
                                         a.flow_canonical[2 * p + 1], 0, g0, g1);
            a.flow_global[2 * p] = g0;
            a.flow_global[2 * p + 1] = g1;
            const double wx = (double)fmaf(g1, r01, g0 * r00) + ftx;
            const double wy = (double)fmaf(g1, r11, g0 * r10) + fty;
            a.flow_world[2 * p] = wx;
            a.flow_world[2 * p + 1] = wy;
            double cr, cg, cb;
            flow_colour(wx, wy, cr, cg, cb);
            a.rgb[3 * p] = cr;
            a.rgb[3 * p + 1] = cg;
            a.rgb[3 * p + 2] = cb;
            s_v[0][j] = wx;
            s_v[1][j] = wy;
            s_v[2][j] = cr;
            s_v[3][j] = cg;
            s_v[4][j] = cb;
            s_id[j] = a.instance_mask[p];
        }
        pof_lds_order<THREADS>();
        row_sums<THREADS>(s_id, s_v, n, nd, acc, cnt);         // id 0 (no centre) and ids beyond num_det: nobody's
        pof_lds_order<THREADS>();                              // the next chunk overwrites the staged points
    }

#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int k = tid + THREADS * c;
        if (k >= N) continue;
        const long long q = row + k;
        double ox = 0.0, oy = 0.0, f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        int count = 0;
        uint8_t valid = 0;
        if (k < nd) {
            pose.det_to_world(a.det_xy[2 * q], a.det_xy[2 * q + 1], ox, oy);
            count = cnt[c];
            const double m = (double)count;                    // 0 / 0 -> NaN, like np.mean of nothing
#pragma unroll
            for (int j = 0; j < 5; ++j) f[j] = acc[c][j] / m;
            valid = a.det_cls[q] >= a.cls_thresh ? 1 : 0;
        }
        a.det_xy_world[2 * q] = ox;
        a.det_xy_world[2 * q + 1] = oy;
        a.det_flow[2 * q] = f[0];
        a.det_flow[2 * q + 1] = f[1];
        a.det_rgb[3 * q] = f[2];
        a.det_rgb[3 * q + 1] = f[3];
        a.det_rgb[3 * q + 2] = f[4];
        a.det_count[q] = count;
        a.det_valid[q] = valid;
    }
}

}  // namespace

extern "C" int pof_person_flow(const float *flow_canonical, const double *tab, const int32_t *instance_mask,
                               const int32_t *num_det, const double *det_xy, const double *det_cls,
                               const float *rot, const double *trans, const double *flow_trans,
                               double cls_thresh, int B, int N, float *flow_global, double *flow_world,
                               double *rgb, double *det_xy_world, double *det_flow, double *det_rgb,
                               int32_t *det_count, uint8_t *det_valid, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!flow_canonical || !tab || !instance_mask || !num_det || !det_xy || !det_cls || !rot || !trans ||
        !flow_trans || !flow_global || !flow_world || !rgb || !det_xy_world || !det_flow || !det_rgb ||
        !det_count || !det_valid)
        return POF_E_BADARG;
    if (B < 0 || N < 1) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_nms_predicted_center
    if (B == 0) return POF_OK;
    PersonFlowArgs a;
    a.flow_canonical = flow_canonical; a.tab = tab; a.instance_mask = instance_mask; a.num_det = num_det;
    a.det_xy = det_xy; a.det_cls = det_cls; a.rot = rot; a.trans = trans; a.flow_trans = flow_trans;
    a.cls_thresh = cls_thresh; a.N = N;
    a.flow_global = flow_global; a.flow_world = flow_world; a.rgb = rgb; a.det_xy_world = det_xy_world;
    a.det_flow = det_flow; a.det_rgb = det_rgb; a.det_count = det_count; a.det_valid = det_valid;
    POF_LAUNCH_PER_SENSOR(person_flow_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
