// The tile form of the occupancy grid (N12), shared by the launches that walk its cells: grid_map.hip (N12) and
// grid_scroll.hip (N14).  A grid is H x W int16 cells per sensor, H and W multiples of kTile in [kMinSide, kMaxSide]; a
// row of a tile is one 128-byte line, a workgroup of kCellThreads threads owns one tile, a thread kRun neighbouring
// cells of a row (one 16-byte load and store) in each of its kTile / (kCellThreads / (kTile / kRun)) passes.
#pragma once

namespace pof_grid {

constexpr int kTile = 64;                       // cells per tile side: a row of int16 is one 128-byte line
constexpr int kCellThreads = 256;
constexpr int kRun = 8;                         // neighbouring cells per thread: 16 bytes
constexpr int kRowsPerPass = kCellThreads / (kTile / kRun);
constexpr int kMinSide = 64, kMaxSide = 2048;

}  // namespace pof_grid
