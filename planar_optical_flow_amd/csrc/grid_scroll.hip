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
#include "pof_grid.h"

namespace {

using namespace pof_grid;

__global__ __launch_bounds__(kCellThreads) void grid_scroll_stage_kernel(ScrollArgs a, int tiles_x, int tiles)
{
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const TileThread me(tiles_x, tiles);
    const int b = me.b;
    int sx, sy;
    scroll_shift(a, b, sx, sy);
    if (me.tile == 0 && tid == 0) scroll_write_shift(a, b, sx, sy);
    if ((sx | sy) == 0) return;

    int ux, uy;                                                                // the source tile
    const bool inside = scroll_source(me, tiles_x, tiles, sx, sy, ux, uy);
    for (int pass = 0; pass < kTile; pass += kRowsPerPass) {
        uint4 cells = make_uint4(0u, 0u, 0u, 0u);                              // unknown
        if (inside) cells = *reinterpret_cast<const uint4 *>(a.grid + me.run(H, W, ux, uy, pass));
        *reinterpret_cast<uint4 *>(a.scratch + me.run(H, W, me.tx, me.ty, pass)) = cells;
    }
}

__global__ __launch_bounds__(kCellThreads) void grid_scroll_commit_kernel(ScrollArgs a, int tiles_x, int tiles)
{
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const TileThread me(tiles_x, tiles);
    const int b = me.b;
    const int sx = a.shift[2 * b], sy = a.shift[2 * b + 1];
    if ((sx | sy) == 0) return;

    if (me.tile == 0 && tid == 0) scroll_write_origin(a, b, sx, sy);
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
    const ScrollArgs a = {trans, res, margin, H, W, grid, origin, base, offset, scratch, shift, scrolled};
    const int refused = scroll_check(a, B);
    if (refused != POF_OK || B == 0) return refused;
    const Tiles tiles(H, W);
    grid_scroll_stage_kernel<<<B * tiles.all, kCellThreads, 0, pof_stream(stream)>>>(a, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    grid_scroll_commit_kernel<<<B * tiles.all, kCellThreads, 0, pof_stream(stream)>>>(a, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
