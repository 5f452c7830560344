// N12: occupancy grid map, a per-sensor int16 log-odds grid updated per scan.  One entry point, two launches on the
// caller's stream; include/pof_abi.h has the contract.
//
// (a) grid_points_kernel, the per-sensor workgroup of pof_sensor.h: per beam the endpoint in the world frame by N11's
//     expression (SensorPose), its cell (pof_grid.h's Cell), the grid value there as the grid stands -- the cells launch
//     runs behind it on the stream -- and whether the beam marks its cell (a hit inside the grid that is no person's
//     point, pof_ego_motion's gate: NmsGate).  det_points / det_free are counted with integer LDS atomics: integer sums
//     have no order.
// (b) grid_cells_kernel, the tile form of pof_grid.h.  The tile's hit flags are staged in LDS from point_cell /
//     point_mark (N int32 + N uint8 from L2; no float64 of the points is redone per tile), the ranges as float32 next
//     to them, and every thread applies the cell rule to its cells: +hit where a flag is set, else -miss when the cell's
//     beam and its two neighbours all see past the cell, else nothing.  A thread stores only when one of its 8 cells
//     changed.
//
// No global atomics and no order-dependent sum: the same bits in every run, at every batch position and in a replay.
//
// Early exits of a tile, both decided from the sensor's 12 scalars (rot, trans, origin) before any other global access
// and both exact by the monotonicity of IEEE multiplies, adds, divides, floor and sqrt (x <= y gives fl(x op c) <=
// fl(y op c) for every rounding-to-nearest op with a fixed c of fixed sign):
//   * no cell can be freed: s_x = R00 d_x + R10 d_y, as the cell rule computes it, is monotone in d_x and in d_y, and
//     d_x, d_y are monotone in the cell index, so over the tile s_x lies between the smallest and the largest of its four
//     corner values; lb_x = their distance from 0 (0 when they straddle it or one is NaN), lb_y likewise, and every
//     cell has rho >= sqrt(lb_x lb_x + lb_y lb_y) =: rho_lb in the kernel's own arithmetic.  Rule 2 needs rho + tol < f
//     with f <= max_range, so rho_lb + tol >= max_range rules it out for the whole tile.
//   * no endpoint can fall into the tile: a hit has r < max_range and the table's |cos|, |sin| <= 1, so |p_x|, |p_y| <
//     max_range, |R00 p_x + R01 p_y| <= |R00| max_range + |R01| max_range =: e_x (same operations, larger operands), w_x
//     lies in [t_x - e_x, t_x + e_x] and g_x between the g of those two; likewise y.  A tile outside that box of cells
//     holds no endpoint.  A NaN anywhere fails the comparison and the tile is kept.
//   A tile with neither leaves at once; one without frees skips the float64 work, one without endpoints the staging.
// A tile wholly outside the field of view is not detected (not built).
#include <cmath>

#include "pof_grid.h"
#include "pof_sensor.h"

namespace {

using namespace pof_sensor;
using namespace pof_grid;

struct GridMapArgs {
    const float *ranges;
    const double *tab;
    const float *rot;
    const double *trans;
    NmsGate gate;
    double res, tol, max_range;
    int hit, miss, lo, hi, free_thresh, N, H, W;
    int16_t *grid;
    const double *origin;
    int32_t *point_cell;
    uint8_t *point_mark;
    int16_t *point_prior;
    int32_t *det_points, *det_free;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void grid_points_kernel(GridMapArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ int s_points[kMaxN], s_free[kMaxN];
    const int N = a.N, H = a.H, W = a.W, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const int nd = a.gate.num(b, N);
    const SensorPose pose(a.rot, a.trans, b);
    const double ox = a.origin[2 * b], oy = a.origin[2 * b + 1];
    const int16_t *grid = a.grid + (long long)b * H * W;

    for (int k = tid; k < N; k += THREADS) s_points[k] = s_free[k] = 0;
    pof_lds_order<THREADS>();
    for (int i = tid; i < N; i += THREADS) {
        const double r = (double)a.ranges[row + i];
        double wx, wy;
        pose.point_to_world(r * a.tab[N + 2 * i], r * a.tab[N + 2 * i + 1], wx, wy);
        const Cell g = Cell::of(wx, wy, ox, oy, a.res);
        const bool inside = is_hit(r, a.max_range) && g.within(0, H, W);
        const int cell = inside ? g.index(W) : -1;
        const int prior = inside ? (int)grid[cell] : -32768;
        const int id = a.gate.id_of(row, i);
        const int k = a.gate.row_of(id, nd);
        const bool person = a.gate.id_is_person(row, id, nd);
        a.point_cell[row + i] = cell;
        a.point_prior[row + i] = (int16_t)prior;
        a.point_mark[row + i] = inside && !person ? 1 : 0;
        if (inside && k >= 0) {
            atomicAdd(&s_points[k], 1);
            if (prior <= -a.free_thresh) atomicAdd(&s_free[k], 1);
        }
    }
    pof_lds_order<THREADS>();
    for (int k = tid; k < N; k += THREADS) {
        a.det_points[row + k] = k < nd ? s_points[k] : 0;
        a.det_free[row + k] = k < nd ? s_free[k] : 0;
    }
}

// the distance from 0 of the interval the four corner values span: 0 when they straddle 0 or one is NaN
__device__ __forceinline__ double corner_bound(double v0, double v1, double v2, double v3)
{
    if (v0 > 0.0 && v1 > 0.0 && v2 > 0.0 && v3 > 0.0) return fmin(fmin(v0, v1), fmin(v2, v3));
    if (v0 < 0.0 && v1 < 0.0 && v2 < 0.0 && v3 < 0.0) return -fmax(fmax(v0, v1), fmax(v2, v3));
    return 0.0;
}

__global__ __launch_bounds__(kCellThreads) void grid_cells_kernel(GridMapArgs a, int tiles_x, int tiles)
{
    __shared__ float s_r[kGroupMaxN];                          // the scan; only beams inside [0, N) are read
    __shared__ uint8_t s_hit[kTile * kTile];
    const int N = a.N, H = a.H, W = a.W, tid = threadIdx.x;
    const TileThread me(tiles_x, tiles);
    const int b = me.b, x0 = me.tx * kTile, y0 = me.ty * kTile, lx0 = me.lx0;
    const long long row = (long long)b * N;
    const SensorPose pose(a.rot, a.trans, b);
    const double tx = pose.tx, ty = pose.ty;
    const double ox = a.origin[2 * b], oy = a.origin[2 * b + 1];
    const double res = a.res, max_range = a.max_range;

    // the two early exits (see the head of the file); every value here is the same in all threads
    bool can_free, can_hit;
    {
        const double dxa = (ox + ((double)x0 + 0.5) * res) - tx, dxb = (ox + ((double)(x0 + kTile - 1) + 0.5) * res) - tx;
        const double dya = (oy + ((double)y0 + 0.5) * res) - ty, dyb = (oy + ((double)(y0 + kTile - 1) + 0.5) * res) - ty;
        double cx[4], cy[4];                                   // the tile's corners in the sensor frame
#pragma unroll
        for (int q = 0; q < 4; ++q) pose.to_sensor(q & 2 ? dxb : dxa, q & 1 ? dyb : dya, cx[q], cy[q]);
        const double lbx = corner_bound(cx[0], cx[1], cx[2], cx[3]), lby = corner_bound(cy[0], cy[1], cy[2], cy[3]);
        const double rho_lb = sqrt(lbx * lbx + lby * lby);
        can_free = !(rho_lb + a.tol >= max_range);
        const double ex = fabs((double)pose.r00) * max_range + fabs((double)pose.r01) * max_range;
        const double ey = fabs((double)pose.r10) * max_range + fabs((double)pose.r11) * max_range;
        const double gxa = floor(((tx - ex) - ox) / res), gxb = floor(((tx + ex) - ox) / res);
        const double gya = floor(((ty - ey) - oy) / res), gyb = floor(((ty + ey) - oy) / res);
        can_hit = !(gxb < (double)x0 || gxa > (double)(x0 + kTile - 1) || gyb < (double)y0 ||
                    gya > (double)(y0 + kTile - 1));
    }
    if (!can_free && !can_hit) return;

    if (can_hit) {
        for (int j = tid; j < kTile * kTile / 4; j += kCellThreads) reinterpret_cast<uint32_t *>(s_hit)[j] = 0u;
        __syncthreads();
        for (int i = tid; i < N; i += kCellThreads) {
            const int cell = a.point_cell[row + i];
            if (cell < 0 || !a.point_mark[row + i]) continue;
            const int lx = cell % W - x0, ly = cell / W - y0;
            if (lx >= 0 && lx < kTile && ly >= 0 && ly < kTile) s_hit[ly * kTile + lx] = 1;    // every writer writes 1
        }
    }
    if (can_free)
        for (int i = tid; i < N; i += kCellThreads) s_r[i] = a.ranges[row + i];
    __syncthreads();

    const double phi0 = a.tab[0], dphi = N > 1 ? a.tab[1] - phi0 : 0.0;
    for (int pass = 0; pass < kTile; pass += kRowsPerPass) {
        const int ly = pass + me.ly0, iy = y0 + ly;
        int16_t *at = a.grid + me.run(H, W, me.tx, me.ty, pass);
        union {
            uint4 q;
            int16_t v[kRun];
        } cells;
        cells.q = *reinterpret_cast<const uint4 *>(at);
        bool changed = false;
        const double dy = (oy + ((double)iy + 0.5) * res) - ty;
#pragma unroll
        for (int c = 0; c < kRun; ++c) {
            int delta = 0;
            if (can_hit && s_hit[ly * kTile + lx0 + c]) {
                delta = a.hit;
            } else if (can_free) {
                const double dx = (ox + ((double)(x0 + lx0 + c) + 0.5) * res) - tx;
                double sx, sy;
                pose.to_sensor(dx, dy, sx, sy);
                const double rho = sqrt(sx * sx + sy * sy);
                const double t = rint((atan2(sy, sx) - phi0) / dphi);
                if (t >= 0.0 && t < (double)N) {               // a NaN and an infinity are outside
                    const int m = (int)t;
                    const double rm = (double)s_r[m];
                    if (rm > 0.0) {                            // beam m is valid: not NaN, > 0
                        double f = fmin(rm, max_range);
                        if (m > 0) {
                            const double rn = (double)s_r[m - 1];
                            if (rn > 0.0) f = fmin(f, fmin(rn, max_range));
                        }
                        if (m + 1 < N) {
                            const double rn = (double)s_r[m + 1];
                            if (rn > 0.0) f = fmin(f, fmin(rn, max_range));
                        }
                        if (rho + a.tol < f) delta = -a.miss;
                    }
                }
            }
            if (delta != 0) {
                int v = (int)cells.v[c] + delta;
                v = v < a.lo ? a.lo : (v > a.hi ? a.hi : v);
                changed = changed || v != (int)cells.v[c];
                cells.v[c] = (int16_t)v;
            }
        }
        if (changed) *reinterpret_cast<uint4 *>(at) = cells.q;
    }
}

}  // namespace

extern "C" int pof_grid_map_update(const float *ranges, const double *tab, const float *rot, const double *trans,
                                   const int32_t *instance_mask, const int32_t *num_det, const double *det_cls,
                                   double res, double tol, double max_range, double cls_thresh, int hit, int miss,
                                   int lo, int hi, int free_thresh, int B, int N, int H, int W, int16_t *grid,
                                   const double *origin, int32_t *point_cell, uint8_t *point_mark,
                                   int16_t *point_prior, int32_t *det_points, int32_t *det_free, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges || !tab || !rot || !trans || !grid || !origin || !point_cell || !point_mark || !point_prior ||
        !det_points || !det_free)
        return POF_E_BADARG;
    if (!nms_gate_ok(instance_mask, num_det, det_cls)) return POF_E_BADARG;
    if (!(res > 0.0) || !(tol >= 0.0) || !(max_range > 0.0) || hit < 0 || miss < 0 || lo < -32767 || lo > 0 ||
        hi < 0 || hi > 32767 || free_thresh < 0 || B < 0 || N < 1)
        return POF_E_BADARG;
    if (N > kGroupMaxN || !shape_ok(H, W)) return POF_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(grid) % 16) return POF_E_SHAPE;           // the cells launch moves 16 bytes at a time
    const Tiles tiles(H, W);
    if (!tiles.fit(B)) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    GridMapArgs a;
    a.ranges = ranges; a.tab = tab; a.rot = rot; a.trans = trans; a.gate = {instance_mask, num_det, det_cls, cls_thresh};
    a.res = res; a.tol = tol; a.max_range = max_range; a.hit = hit;
    a.miss = miss; a.lo = lo; a.hi = hi; a.free_thresh = free_thresh; a.N = N; a.H = H; a.W = W; a.grid = grid;
    a.origin = origin; a.point_cell = point_cell; a.point_mark = point_mark; a.point_prior = point_prior;
    a.det_points = det_points; a.det_free = det_free;
    POF_LAUNCH_PER_SENSOR(grid_points_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    grid_cells_kernel<<<B * tiles.all, kCellThreads, 0, pof_stream(stream)>>>(a, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
