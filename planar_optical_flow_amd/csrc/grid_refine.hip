// N19: grid refine, a sub-cell Gauss-Newton fit of the pose to the occupancy grid of N12 -- the scan's endpoints against
// the bilinearly interpolated, clamped log-odds, every scan, behind the pose launch (and behind N13 where that runs).
// One entry point, one launch on the caller's stream; include/pof_abi.h has the contract, tests/test_grid_refine.py
// restates it in float64 NumPy, the order of the sums included.
//
// grid_refine_kernel<THREADS>, the per-sensor workgroup of pof_sensor.h (one wave up to N = 512, 512 threads up to
// 4096).  Thread t keeps p = r (cos, sin) of its kSlots points in registers; an evaluation at (x, y, phi) turns and
// shifts them, gathers the four int16 cells around each (a cell outside the grid is a load of cell 0 that is thrown
// away, so the walk has no branch around a load), and adds the eleven products in slot order; the sums meet in
// group_sum<THREADS, 11>, which leaves the same bits in every lane.  Every lane then solves the 3 x 3 system
// redundantly (pof_icp.h's cholesky3, shared with the ICP) and takes the same exit, so the loop is wave-uniform and
// needs no broadcast.  Thread 0 applies the gates and writes the outputs, and with `moved` the pose and its terms
// (pof_write_pose_terms).
//
// The gathers are divergent by nature: neighbouring beams end a few cells apart along a wall, so a wave's 64 x 4 loads
// fall into a handful of 128-byte lines of two grid rows each, and the grid of one sensor (128 KB at 256 x 256) stays
// in L2 between the evaluations.  No atomics, no libm call but the one sincos per evaluation, FIXED ORDER of every sum
// (pof_sensor.h): the same bits in every run, at every batch position and in a replay.
#include <cmath>

#include "pof_grid.h"
#include "pof_icp.h"
#include "pof_sensor.h"

namespace {

using namespace pof_sensor;

constexpr int kRefineSums = 11;
constexpr int kRefineMaxIters = 32, kRefineMaxCap = 32767;

struct GridRefineArgs {
    const float *ranges;
    const double *tab;
    NmsGate gate;
    double max_range;
    const int16_t *grid;
    const double *origin;
    double res, min_pivot, max_shift, max_turn, eps_shift, eps_turn;
    int cap, iters, min_points, N, H, W;
    double *pose;
    float *rot;
    double *trans;
    double *correction, *score, *obs;
    int32_t *votes, *count, *iters_used;
    uint8_t *ok, *moved;
};

// m(i, j): the cell clamped to [-cap, cap] over cap, 0 outside the grid; the load itself is always inside
__device__ __forceinline__ double cell_value(const int16_t *grid, int i, int j, int H, int W, int cap, double capd)
{
    const bool inside = (unsigned)i < (unsigned)W && (unsigned)j < (unsigned)H;
    int v = (int)grid[inside ? j * W + i : 0];
    v = v < -cap ? -cap : (v > cap ? cap : v);
    return inside ? (double)v / capd : 0.0;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void grid_refine_kernel(GridRefineArgs a)
{
    __shared__ double s_part[kRefineSums * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, H = a.H, W = a.W, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const int nd = a.gate.num(b, N);
    const int16_t *grid = a.grid + (long long)b * H * W;
    const double ox = a.origin[2 * b], oy = a.origin[2 * b + 1], res = a.res, capd = (double)a.cap;
    const double x_in = a.pose[3 * b], y_in = a.pose[3 * b + 1], phi_in = a.pose[3 * b + 2];

    double px[kSlots], py[kSlots];
    bool vote[kSlots];
    double V[1] = {0.0};
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = tid + THREADS * c;
        px[c] = py[c] = 0.0;
        vote[c] = false;
        if (i < N) {
            const double r = (double)a.ranges[row + i];
            if (is_hit(r, a.max_range) && !a.gate.is_person(row, i, nd)) {
                px[c] = r * a.tab[N + 2 * i];
                py[c] = r * a.tab[N + 2 * i + 1];
                vote[c] = true;
                V[0] += 1.0;
            }
        }
    }
    group_sum<THREADS, 1>(V, s_part);
    const int votes = (int)V[0];

    const double qnan = __builtin_nan("");
    double cx = 0.0, cy = 0.0, ct = 0.0, s0 = qnan, s1 = qnan, obs = 0.0;
    int used = 0, count = 0;
    bool ok = votes >= a.min_points, last = false, first = true;
    for (;;) {                                                 // uniform: every thread holds the same bits
        const double x = x_in + cx * res, y = y_in + cy * res, phi = phi_in + ct;
        double sn, cs;
        sincos(phi, &sn, &cs);
        double S[kRefineSums];
#pragma unroll
        for (int k = 0; k < kRefineSums; ++k) S[k] = 0.0;
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            if (!vote[c]) continue;
            const double dx = cs * px[c] - sn * py[c], dy = sn * px[c] + cs * py[c];
            const double u = pof_grid::cell_coord(dx + x, ox, res) - 0.5, v = pof_grid::cell_coord(dy + y, oy, res) - 0.5;
            const double i0 = floor(u), j0 = floor(v);
            if (!(i0 >= -1.0 && i0 < (double)W && j0 >= -1.0 && j0 < (double)H)) continue;     // a NaN is outside
            const int ii = (int)i0, jj = (int)j0;
            const double fx = u - i0, fy = v - j0;
            const double m00 = cell_value(grid, ii, jj, H, W, a.cap, capd);
            const double m10 = cell_value(grid, ii + 1, jj, H, W, a.cap, capd);
            const double m01 = cell_value(grid, ii, jj + 1, H, W, a.cap, capd);
            const double m11 = cell_value(grid, ii + 1, jj + 1, H, W, a.cap, capd);
            const double M = (m00 * (1.0 - fx) + m10 * fx) * (1.0 - fy) + (m01 * (1.0 - fx) + m11 * fx) * fy;
            const double gx = (m10 - m00) * (1.0 - fy) + (m11 - m01) * fy;
            const double gy = (m01 - m00) * (1.0 - fx) + (m11 - m10) * fx;
            const double lx = dx / res, ly = dy / res;
            const double j0_ = gx, j1_ = gy, j2_ = gy * lx - gx * ly, e = 1.0 - M;
            S[0] += j0_ * j0_;
            S[1] += j0_ * j1_;
            S[2] += j0_ * j2_;
            S[3] += j1_ * j1_;
            S[4] += j1_ * j2_;
            S[5] += j2_ * j2_;
            S[6] += j0_ * e;
            S[7] += j1_ * e;
            S[8] += j2_ * e;
            S[9] += M;
            S[10] += 1.0;
        }
        group_sum<THREADS, kRefineSums>(S, s_part);
        const int n = (int)S[10];
        if (first) {
            first = false;
            count = n;
            s0 = S[9] / S[10];
        }
        if (n < a.min_points) ok = false;
        if (!ok) break;
        if (last) {
            s1 = S[9] / S[10];
            break;
        }
        const pof_icp::Solve3 sol = pof_icp::cholesky3(S[0], S[1], S[2], S[3], S[4], S[5], -S[6], -S[7], -S[8], a.min_pivot);
        obs = sol.obs;
        if (sol.failed) {
            ok = false;
            break;
        }
        cx = cx + sol.x0;
        cy = cy + sol.x1;
        ct = ct + sol.x2;
        ++used;
        last = used == a.iters || (fmax(fabs(sol.x0), fabs(sol.x1)) < a.eps_shift && fabs(sol.x2) < a.eps_turn);
    }
    if (tid != 0) return;
    const bool moved = ok && fmax(fabs(cx), fabs(cy)) <= a.max_shift && fabs(ct) <= a.max_turn && s1 > s0;
    a.votes[b] = votes;
    a.count[b] = count;
    a.iters_used[b] = used;
    a.ok[b] = ok ? 1 : 0;
    a.moved[b] = moved ? 1 : 0;
    a.obs[b] = obs;
    a.score[2 * b] = s0;
    a.score[2 * b + 1] = ok ? s1 : qnan;
    double mx = 0.0, my = 0.0, mt = 0.0;
    if (moved) {
        mx = cx * res;
        my = cy * res;
        mt = ct;
        const double x = x_in + cx * res, y = y_in + cy * res, phi = phi_in + ct;
        a.pose[3 * b] = x;
        a.pose[3 * b + 1] = y;
        a.pose[3 * b + 2] = phi;
        pof_write_pose_terms(b, x, y, phi, 0.0, 0.0, a.rot, a.trans, nullptr);
    }
    a.correction[3 * b] = mx;
    a.correction[3 * b + 1] = my;
    a.correction[3 * b + 2] = mt;
}

}  // namespace

extern "C" int pof_grid_refine(const float *ranges, const double *tab, const int32_t *instance_mask,
                               const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range,
                               const int16_t *grid, const double *origin, double res, int cap, int iters,
                               int min_points, double min_pivot, double max_shift, double max_turn, double eps_shift,
                               double eps_turn, int B, int N, int H, int W, double *pose, float *rot, double *trans,
                               double *correction, double *score, double *obs, int32_t *votes, int32_t *count,
                               int32_t *iters_used, uint8_t *ok, uint8_t *moved, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges || !tab || !grid || !origin || !pose || !rot || !trans || !correction || !score || !obs || !votes ||
        !count || !iters_used || !ok || !moved)
        return POF_E_BADARG;
    if (!nms_gate_ok(instance_mask, num_det, det_cls)) return POF_E_BADARG;
    if (!(res > 0.0) || !(max_range > 0.0) || cap < 1 || cap > kRefineMaxCap || iters < 1 || iters > kRefineMaxIters ||
        min_points < 0 || !(min_pivot >= 0.0) || !(max_shift >= 0.0) || !(max_turn >= 0.0) || B < 0 || N < 1)
        return POF_E_BADARG;
    if (N > kGroupMaxN || !pof_grid::shape_ok(H, W)) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    GridRefineArgs a;
    a.ranges = ranges; a.tab = tab; a.gate = {instance_mask, num_det, det_cls, cls_thresh}; a.max_range = max_range;
    a.grid = grid; a.origin = origin; a.res = res; a.min_pivot = min_pivot; a.max_shift = max_shift;
    a.max_turn = max_turn; a.eps_shift = eps_shift; a.eps_turn = eps_turn; a.cap = cap; a.iters = iters;
    a.min_points = min_points; a.N = N; a.H = H; a.W = W; a.pose = pose; a.rot = rot; a.trans = trans;
    a.correction = correction; a.score = score; a.obs = obs; a.votes = votes; a.count = count;
    a.iters_used = iters_used; a.ok = ok; a.moved = moved;
    POF_LAUNCH_PER_SENSOR(grid_refine_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
