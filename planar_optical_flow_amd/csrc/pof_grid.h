// The occupancy grid of the map stages, defined once: grid_map.hip (N12), grid_match.hip (N13), grid_scroll.hip (N14),
// grid_cast.hip (N16) and grid_store.hip (N20).  A grid is H x W int16 cells per sensor, H and W multiples of kTile in [kMinSide, kMaxSide].
// The launches that walk all cells (N12's cells launch, N14) have the tile form: a row of a tile is one 128-byte line, a
// workgroup of kCellThreads threads owns one tile, a thread kRun neighbouring cells of a row (one 16-byte load and
// store) in each of its kTile / kRowsPerPass passes.
#pragma once
#include <cmath>

#include "pof_common.h"

namespace pof_grid {

constexpr int kTile = 64;                       // cells per tile side: a row of int16 is one 128-byte line
constexpr int kCellThreads = 256;
constexpr int kRun = 8;                         // neighbouring cells per thread: 16 bytes
constexpr int kRowsPerPass = kCellThreads / (kTile / kRun);
constexpr int kMinSide = 64, kMaxSide = 2048;

// the rule for H and W; a launcher answers POF_E_SHAPE without it
inline bool shape_ok(int H, int W)
{
    return !(H < kMinSide || H > kMaxSide || W < kMinSide || W > kMaxSide || H % kTile || W % kTile);
}

// the workgroups of a tile launch over B grids: B * all of them
struct Tiles {
    int x, all;
    Tiles(int H, int W) : x(W / kTile), all(x * (H / kTile)) {}
    bool fit(int B) const { return (long long)B * all <= 0x7fffffffLL; }
};

// one axis of a world point in cells, not yet floored: w the point, o the grid's origin.  A true division.
__device__ __forceinline__ double cell_coord(double w, double o, double res) { return (w - o) / res; }

// The cell of a world point: the two floored quotients, kept and compared in double, so a NaN, an infinity and
// whatever an int could not hold are outside.
struct Cell {
    double gx, gy;

    __device__ __forceinline__ static Cell of(double wx, double wy, double ox, double oy, double res)
    {
        return {floor(cell_coord(wx, ox, res)), floor(cell_coord(wy, oy, res))};
    }

    // at most `reach` cells outside the grid; 0: inside it
    __device__ __forceinline__ bool within(int reach, int H, int W) const
    {
        return gx >= (double)-reach && gx < (double)(W + reach) && gy >= (double)-reach && gy < (double)(H + reach);
    }

    __device__ __forceinline__ int index(int W) const { return (int)gy * W + (int)gx; }       // of a cell inside
};

// Where a thread of a tile launch works: sensor b, tile (tx, ty) in tiles, and in every pass (kTile / kRowsPerPass of
// them, kRowsPerPass rows apart) the kRun cells from column lx0 of the tile's row pass + ly0.
struct TileThread {
    int b, tile, tx, ty, lx0, ly0;

    __device__ __forceinline__ TileThread(int tiles_x, int tiles)
    {
        const int tid = threadIdx.x;
        b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
        tx = tile % tiles_x, ty = tile / tiles_x;
        lx0 = (tid % (kTile / kRun)) * kRun, ly0 = tid / (kTile / kRun);
    }

    // where the thread's run of a pass in tile (at_x, at_y) of its sensor starts in a [B,H,W] array: 16-byte aligned
    __device__ __forceinline__ long long run(int H, int W, int at_x, int at_y, int pass) const
    {
        return ((long long)b * H + at_y * kTile + pass + ly0) * W + at_x * kTile + lx0;
    }
};

// ---- the scroll rule of N14, shared by grid_scroll.hip and grid_store.hip (N20)
constexpr double kMaxCell = 1073741824.0;       // 2^30: a sensor cell at or beyond it scrolls nothing
constexpr long long kMaxOffset = 1 << 20;       // |offset| in tiles stays within it

// what both scrolls read and write per sensor
struct ScrollArgs {
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

// the decision of sensor b from eight scalars, the same value in every workgroup of the sensor
__device__ __forceinline__ void scroll_shift(const ScrollArgs &a, int b, int &sx, int &sy)
{
    sx = axis_shift(a.trans[2 * b], a.origin[2 * b], a.res, a.margin, a.W, a.offset[2 * b]);
    sy = axis_shift(a.trans[2 * b + 1], a.origin[2 * b + 1], a.res, a.margin, a.H, a.offset[2 * b + 1]);
}

__device__ __forceinline__ void scroll_write_shift(const ScrollArgs &a, int b, int sx, int sy)
{
    a.shift[2 * b] = sx;
    a.shift[2 * b + 1] = sy;
    a.scrolled[b] = (sx | sy) != 0 ? 1 : 0;
}

// offset += s and the origin from base, not accumulated: a sensor that scrolls away and back gets its origin's old
// bits back
__device__ __forceinline__ void scroll_write_origin(const ScrollArgs &a, int b, int sx, int sy)
{
    const int ox = a.offset[2 * b] + sx, oy = a.offset[2 * b + 1] + sy;
    a.offset[2 * b] = ox;
    a.offset[2 * b + 1] = oy;
    a.origin[2 * b] = a.base[2 * b] + (double)(kTile * ox) * a.res;
    a.origin[2 * b + 1] = a.base[2 * b + 1] + (double)(kTile * oy) * a.res;
}

// the source tile (ux, uy) of the workgroup's DESTINATION tile under the shift -> whether it lies inside the grid; a
// shift is a whole number of tiles, so a destination tile has one source tile, wholly inside or wholly outside
__device__ __forceinline__ bool scroll_source(const TileThread &me, int tiles_x, int tiles, int sx, int sy, int &ux, int &uy)
{
    const long long lx = (long long)me.tx + sx, ly = (long long)me.ty + sy;
    ux = (int)lx, uy = (int)ly;
    return lx >= 0 && lx < tiles_x && ly >= 0 && ly < tiles / tiles_x;
}

// the refusals of N14, in its order; POF_OK: launch (or return at B = 0)
inline int scroll_check(const ScrollArgs &a, int B)
{
    if (!a.trans || !a.grid || !a.origin || !a.base || !a.offset || !a.scratch || !a.shift || !a.scrolled) return POF_E_BADARG;
    if (!(a.res > 0.0) || a.margin < 0 || B < 0) return POF_E_BADARG;
    if (!shape_ok(a.H, a.W)) return POF_E_SHAPE;
    // a re-centred sensor stands on tile TW / 2: the bound keeps it outside the margin
    if (a.margin > kTile * ((a.W / kTile - 1) / 2) || a.margin > kTile * ((a.H / kTile - 1) / 2)) return POF_E_BADARG;
    if (reinterpret_cast<uintptr_t>(a.grid) % 16 || reinterpret_cast<uintptr_t>(a.scratch) % 16) return POF_E_SHAPE;
    if (!Tiles(a.H, a.W).fit(B)) return POF_E_SHAPE;
    return POF_OK;
}

}  // namespace pof_grid
