// The occupancy grid of the map stages, defined once: grid_map.hip (N12), grid_match.hip (N13), grid_scroll.hip (N14)
// and grid_cast.hip (N16).  A grid is H x W int16 cells per sensor, H and W multiples of kTile in [kMinSide, kMaxSide].
// The launches that walk all cells (N12's cells launch, N14) have the tile form: a row of a tile is one 128-byte line, a
// workgroup of kCellThreads threads owns one tile, a thread kRun neighbouring cells of a row (one 16-byte load and
// store) in each of its kTile / kRowsPerPass passes.
#pragma once
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

}  // namespace pof_grid
