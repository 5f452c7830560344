// N14: the occupancy grid of N12 scrolls with its sensor, by whole tiles, on the device.  One entry point, two launches
// on the caller's stream; include/pof_abi.h has the contract.
//
// Both launches have the tile form of pof_grid.h.  A shift is a whole number of tiles, so a destination tile has one
// source tile, wholly inside the grid or wholly outside it, and every row moved is one 128-byte line read and one written.
// (a) grid_scroll_stage_kernel: every workgroup forms the decision of its sensor from trans, origin and offset -- eight
//     scalars, all read only in this launch, the same value in every workgroup of the sensor -- and leaves when nothing
//     moves.  Otherwise it writes its DESTINATION tile into scratch: the source tile of grid, or zeros where that lies
//     outside.  Tile 0 writes shift and scrolled.
// (b) grid_scroll_commit_kernel: every workgroup reads shift, which (a) wrote, and nothing else; with a shift it copies
//     its tile of scratch back into grid, and tile 0 writes offset and origin.
// Neither launch reads what another workgroup of the same launch writes: (a) reads grid, origin and offset and writes
// scratch, shift and scrolled; (b) reads shift and scratch and writes grid, offset and origin.  No atomics, no sums:
// the same bits in every run, at every batch position and in a replay.  A step without a scroll costs the scalar loads
// and one exit per workgroup, twice.
//
// In place, without the scratch copy, a tile would be read by one workgroup and written by another of the same launch;
// the order of workgroups is not the launch's to choose, so that form is not built.
#include <cmath>

#include "pof_grid.h"

namespace {

using namespace pof_grid;

constexpr double kMaxCell = 1073741824.0;       // 2^30: a sensor cell at or beyond it scrolls nothing
constexpr long long kMaxOffset = 1 << 20;       // |offset| in tiles stays within it

struct GridScrollArgs {
    const double *trans;
    double res;
    int margin, H, W;
    int16_t *grid;
    double *origin;
    const double *base;
    int32_t *offset;
    int16_t *scratch;
    int32_t *shift;
    uint8_t *scrolled;
};

// the shift of one axis in tiles: t the sensor, o the origin, side the cells of the axis, off the offset so far
__device__ __forceinline__ int axis_shift(double t, double o, double res, int margin, int side, int off)
{
    const double c = floor(cell_coord(t, o, res));
    if (!(fabs(c) < kMaxCell)) return 0;                        // a NaN and an infinity included
    const int ci = (int)c;
    if (ci >= margin && ci < side - margin) return 0;
    const int q = ci >= 0 ? ci / kTile : -((kTile - 1 - ci) / kTile);         // floor division
    const int s = q - (side / kTile) / 2;
    const long long to = (long long)off + s;
    return to > kMaxOffset || to < -kMaxOffset ? 0 : s;
}

__global__ __launch_bounds__(kCellThreads) void grid_scroll_stage_kernel(GridScrollArgs a, int tiles_x, int tiles)
{
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const TileThread me(tiles_x, tiles);
    const int b = me.b;
    const int sx = axis_shift(a.trans[2 * b], a.origin[2 * b], a.res, a.margin, W, a.offset[2 * b]);
    const int sy = axis_shift(a.trans[2 * b + 1], a.origin[2 * b + 1], a.res, a.margin, H, a.offset[2 * b + 1]);
    if (me.tile == 0 && tid == 0) {
        a.shift[2 * b] = sx;
        a.shift[2 * b + 1] = sy;
        a.scrolled[b] = (sx | sy) != 0 ? 1 : 0;
    }
    if ((sx | sy) == 0) return;

    const long long ux = (long long)me.tx + sx, uy = (long long)me.ty + sy;    // the source tile
    const bool inside = ux >= 0 && ux < tiles_x && uy >= 0 && uy < tiles / tiles_x;
    for (int pass = 0; pass < kTile; pass += kRowsPerPass) {
        uint4 cells = make_uint4(0u, 0u, 0u, 0u);                              // unknown
        if (inside) cells = *reinterpret_cast<const uint4 *>(a.grid + me.run(H, W, (int)ux, (int)uy, pass));
        *reinterpret_cast<uint4 *>(a.scratch + me.run(H, W, me.tx, me.ty, pass)) = cells;
    }
}

__global__ __launch_bounds__(kCellThreads) void grid_scroll_commit_kernel(GridScrollArgs a, int tiles_x, int tiles)
{
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const TileThread me(tiles_x, tiles);
    const int b = me.b;
    const int sx = a.shift[2 * b], sy = a.shift[2 * b + 1];
    if ((sx | sy) == 0) return;

    if (me.tile == 0 && tid == 0) {
        // from base, not accumulated: a sensor that scrolls away and back gets its origin's old bits back
        const int ox = a.offset[2 * b] + sx, oy = a.offset[2 * b + 1] + sy;
        a.offset[2 * b] = ox;
        a.offset[2 * b + 1] = oy;
        a.origin[2 * b] = a.base[2 * b] + (double)(kTile * ox) * a.res;
        a.origin[2 * b + 1] = a.base[2 * b + 1] + (double)(kTile * oy) * a.res;
    }
    for (int pass = 0; pass < kTile; pass += kRowsPerPass) {
        const long long at = me.run(H, W, me.tx, me.ty, pass);
        *reinterpret_cast<uint4 *>(a.grid + at) = *reinterpret_cast<const uint4 *>(a.scratch + at);
    }
}

}  // namespace

extern "C" int pof_grid_scroll(const double *trans, double res, int margin, int B, int H, int W, int16_t *grid,
                               double *origin, const double *base, int32_t *offset, int16_t *scratch, int32_t *shift,
                               uint8_t *scrolled, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!trans || !grid || !origin || !base || !offset || !scratch || !shift || !scrolled) return POF_E_BADARG;
    if (!(res > 0.0) || margin < 0 || B < 0) return POF_E_BADARG;
    if (!shape_ok(H, W)) return POF_E_SHAPE;
    // a re-centred sensor stands on tile TW / 2: the bound keeps it outside the margin
    if (margin > kTile * ((W / kTile - 1) / 2) || margin > kTile * ((H / kTile - 1) / 2)) return POF_E_BADARG;
    if (reinterpret_cast<uintptr_t>(grid) % 16 || reinterpret_cast<uintptr_t>(scratch) % 16) return POF_E_SHAPE;
    const Tiles tiles(H, W);
    if (!tiles.fit(B)) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    GridScrollArgs a;
    a.trans = trans; a.res = res; a.margin = margin; a.H = H; a.W = W; a.grid = grid; a.origin = origin; a.base = base;
    a.offset = offset; a.scratch = scratch; a.shift = shift; a.scrolled = scrolled;
    grid_scroll_stage_kernel<<<B * tiles.all, kCellThreads, 0, pof_stream(stream)>>>(a, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    grid_scroll_commit_kernel<<<B * tiles.all, kCellThreads, 0, pof_stream(stream)>>>(a, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
