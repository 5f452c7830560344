// N16: the map-predicted scan, a ray cast of the occupancy grid (N12) from the sensor pose, per beam.  One entry point,
// two launches on the caller's stream; include/pof_abi.h has the contract.
//
// (a) grid_cast_walk_kernel, one wave per (sensor, 64 neighbouring beams), one lane per beam: the lane walks its beam
//     through the grid cell by cell (the grid traversal of Amanatides and Woo with the crossings in closed form, X_k =
//     a_x + k q_x), tests every cell it enters and stores the six per-beam outputs and the class of its point.  Which
//     cells a beam enters does not depend on what they hold, so the lane forms the next kAhead steps first, issues their
//     kAhead loads together and only then tests them in order: the chain of dependent 2-byte gathers is a quarter as
//     long as the walk.  Neighbouring lanes read the same cells near the sensor and fan out with range; the trip count
//     differs per lane, and a wave runs as long as its longest beam.  The per-sensor form of pof_sensor.h (one wave per
//     sensor, eight beams per lane in series) would make that chain eight walks long and is not used here.
// (b) grid_cast_counts_kernel, the per-sensor workgroup of pof_sensor.h: the class histogram of the scan and the three
//     counts per detection row, with integer LDS atomics as the points launch of grid_map.hip counts (no order).
//
// No global atomics and no floating-point sum: the same bits in every run, at every batch position and in a replay.
// The walk calls no libm function: multiplies, adds, true divisions and floor.
#include <cmath>

#include "pof_grid.h"
#include "pof_sensor.h"

namespace {

using namespace pof_sensor;
using namespace pof_grid;

constexpr int kAhead = 4;                       // steps formed, and loads issued, before the first of them is tested
constexpr int kBeams = 64;                      // beams per workgroup of the walk: one wave
enum : int { kNone = 0, kOpen = 1, kEdge = 2, kWall = 3, kOutside = 4 };                  // exp_state
enum : int { kClsNone = 0, kClsMap = 1, kClsNovel = 2, kClsThrough = 3, kClsUnknown = 4 };  // point_class

struct GridCastArgs {
    const float *ranges;
    const double *tab;
    const float *rot;
    const double *trans;
    NmsGate gate;
    const int16_t *grid;
    const double *origin;
    double res, max_range, tol;
    int occ_thresh, free_thresh, N, H, W;
    double *exp_range, *exp_far, *free_range;
    int32_t *exp_cell;
    uint8_t *exp_state;
    int32_t *exp_steps;
    uint8_t *point_class;
    int32_t *det_novel, *det_map, *det_through, *class_count;
};

// one axis of a beam: the k-th crossing is at a + (double)k q, +inf for an axis without one
struct Axis {
    double a, q;
    int step;

    __device__ __forceinline__ Axis(double d, double u, double c)
    {
        if (d > 0.0) {
            a = ((c + 1.0) - u) / d, q = 1.0 / d, step = 1;
        } else if (d < 0.0) {
            a = (u - c) / (-d), q = 1.0 / (-d), step = -1;
        } else {                                               // zero or NaN
            a = q = 0.0, step = 0;
        }
    }

    __device__ __forceinline__ double at(int k) const { return step ? a + (double)k * q : INFINITY; }
};

__global__ __launch_bounds__(kBeams) void grid_cast_walk_kernel(GridCastArgs a, int chunks)
{
    const int N = a.N, H = a.H, W = a.W;
    const int b = blockIdx.x / chunks, i = (blockIdx.x - b * chunks) * kBeams + threadIdx.x;
    if (i >= N) return;
    const long long at = (long long)b * N + i;
    const SensorPose pose(a.rot, a.trans, b);
    const double ux = cell_coord(pose.tx, a.origin[2 * b], a.res), uy = cell_coord(pose.ty, a.origin[2 * b + 1], a.res);
    const Cell start = {floor(ux), floor(uy)};                 // the sensor's cell
    const bool inside = start.within(0, H, W);
    const int16_t *grid = a.grid + (long long)b * H * W;

    double exp_range = INFINITY, exp_far = INFINITY, free_range = INFINITY;
    int exp_cell = -1, state = inside ? kNone : kOutside, steps = 0;
    if (inside) {
        const double c = a.tab[N + 2 * i], s = a.tab[N + 2 * i + 1];
        double dx, dy;
        pose.rotate(c, s, dx, dy);
        const Axis ax(dx, ux, start.gx), ay(dy, uy, start.gy);
        int ix = (int)start.gx, iy = (int)start.gy, kx = 0, ky = 0;
        bool done = false, in_run = false, seen = false;
        const int limit = H + W;                               // every step leaves the start by one cell on one axis
        for (int base = 0; base < limit && !done; base += kAhead) {
            double t[kAhead];
            int cell[kAhead];
            int v[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {                 // the steps: no cell value decides them
                const double X = ax.at(kx), Y = ay.at(ky);
                if (X <= Y) {                                  // a corner takes x first
                    t[j] = X, ix += ax.step, ++kx;
                } else {
                    t[j] = Y, iy += ay.step, ++ky;
                }
                if (X == INFINITY && Y == INFINITY) t[j] = INFINITY, cell[j] = -2;       // no crossing at all
                else cell[j] = ix >= 0 && ix < W && iy >= 0 && iy < H ? iy * W + ix : -1;
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) v[j] = cell[j] >= 0 ? (int)grid[cell[j]] : 0;   // the loads, together
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {                 // the tests, in order
                if (done || base + j >= limit) continue;
                if (cell[j] == -2) {
                    done = true;                               // state NONE
                    continue;
                }
                ++steps;
                const double rho = t[j] * a.res;
                if (rho >= a.max_range || cell[j] < 0) {       // (a), then (b)
                    if (in_run) exp_far = rho;
                    else state = rho >= a.max_range ? kOpen : kEdge;
                    done = true;
                    continue;
                }
                if (!in_run && v[j] >= a.occ_thresh) {         // (c)
                    in_run = true, exp_range = rho, exp_cell = cell[j], state = kWall;
                } else if (in_run && v[j] < a.occ_thresh) {
                    exp_far = rho;
                    done = true;
                }
                if (!seen && v[j] > -a.free_thresh) seen = true, free_range = rho;       // (d)
            }
        }
    }

    const double r = (double)a.ranges[at];
    int cls = kClsNone;
    if (is_hit(r, a.max_range) && state != kNone && state != kOutside) {
        if (state == kWall && r >= exp_range - a.tol && r <= exp_far + a.tol) cls = kClsMap;
        else if (state == kWall && r > exp_far + a.tol) cls = kClsThrough;
        else if (r + a.tol < exp_range && r < free_range) cls = kClsNovel;
        else cls = kClsUnknown;
    }
    a.exp_range[at] = exp_range;
    a.exp_far[at] = exp_far;
    a.free_range[at] = free_range;
    a.exp_cell[at] = exp_cell;
    a.exp_state[at] = (uint8_t)state;
    a.exp_steps[at] = steps;
    a.point_class[at] = (uint8_t)cls;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void grid_cast_counts_kernel(GridCastArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ int s_novel[kMaxN], s_map[kMaxN], s_through[kMaxN], s_count[8];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const int nd = a.gate.num(b, N);

    for (int k = tid; k < N; k += THREADS) s_novel[k] = s_map[k] = s_through[k] = 0;
    if (tid < 8) s_count[tid] = 0;
    pof_lds_order<THREADS>();
    for (int i = tid; i < N; i += THREADS) {
        const int cls = a.point_class[row + i];                // the walk launch wrote it: 0..4
        const int k = a.gate.row_of(a.gate.id_of(row, i), nd);
        atomicAdd(&s_count[cls & 7], 1);
        if (k >= 0) {
            if (cls == kClsNovel) atomicAdd(&s_novel[k], 1);
            else if (cls == kClsMap) atomicAdd(&s_map[k], 1);
            else if (cls == kClsThrough) atomicAdd(&s_through[k], 1);
        }
    }
    pof_lds_order<THREADS>();
    for (int k = tid; k < N; k += THREADS) {
        a.det_novel[row + k] = k < nd ? s_novel[k] : 0;
        a.det_map[row + k] = k < nd ? s_map[k] : 0;
        a.det_through[row + k] = k < nd ? s_through[k] : 0;
    }
    if (tid < 5) a.class_count[5 * (long long)b + tid] = s_count[tid];
}

}  // namespace

extern "C" int pof_grid_cast(const float *ranges, const double *tab, const float *rot, const double *trans,
                             const int32_t *instance_mask, const int32_t *num_det, const double *det_cls,
                             const int16_t *grid, const double *origin, double res, double max_range, double tol,
                             int occ_thresh, int free_thresh, int B, int N, int H, int W, double *exp_range,
                             double *exp_far, double *free_range, int32_t *exp_cell, uint8_t *exp_state,
                             int32_t *exp_steps, uint8_t *point_class, int32_t *det_novel, int32_t *det_map,
                             int32_t *det_through, int32_t *class_count, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges || !tab || !rot || !trans || !grid || !origin || !exp_range || !exp_far || !free_range || !exp_cell ||
        !exp_state || !exp_steps || !point_class || !det_novel || !det_map || !det_through || !class_count)
        return POF_E_BADARG;
    if (!nms_gate_ok(instance_mask, num_det, det_cls)) return POF_E_BADARG;
    if (!(res > 0.0) || !(max_range > 0.0) || !(tol >= 0.0) || occ_thresh < 1 || free_thresh < 0 || B < 0 || N < 1)
        return POF_E_BADARG;
    if (N > kGroupMaxN || !shape_ok(H, W)) return POF_E_SHAPE;
    const int chunks = (N + kBeams - 1) / kBeams;
    if ((long long)B * chunks > 0x7fffffffLL) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    GridCastArgs a;
    a.ranges = ranges; a.tab = tab; a.rot = rot; a.trans = trans; a.gate = {instance_mask, num_det, det_cls, 0.0};
    a.grid = grid; a.origin = origin; a.res = res; a.max_range = max_range; a.tol = tol; a.occ_thresh = occ_thresh;
    a.free_thresh = free_thresh; a.N = N; a.H = H; a.W = W; a.exp_range = exp_range; a.exp_far = exp_far;
    a.free_range = free_range; a.exp_cell = exp_cell; a.exp_state = exp_state; a.exp_steps = exp_steps;
    a.point_class = point_class; a.det_novel = det_novel; a.det_map = det_map; a.det_through = det_through;
    a.class_count = class_count;
    grid_cast_walk_kernel<<<B * chunks, kBeams, 0, pof_stream(stream)>>>(a, chunks);
    POF_CHECK_LAUNCH();
    POF_LAUNCH_PER_SENSOR(grid_cast_counts_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
