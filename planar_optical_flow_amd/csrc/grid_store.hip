// N20: N14's scroll with a store of tiles per sensor behind it -- what scrolls out of the window is kept, and a return
// to a mapped place puts the old cells back.  One entry point, three launches on the caller's stream;
// include/pof_abi.h has the contract.  The shift rule, the caps, offset and origin are N14's own code (pof_grid.h).
//
// (a) grid_store_stage_kernel, tile form: as N14's stage launch every workgroup forms the decision of its sensor and
//     writes its DESTINATION tile into scratch.  Where the source lies outside the window the tile ARRIVES: the
//     workgroup searches the sensor's keys and stamps (read only in this launch) for its world tile and fills scratch
//     from the lowest slot found, or with zeros.  The same workgroup looks at its own tile as a SOURCE: where that
//     DEPARTS it ORs its cells.  plan_in[tile] = found slot + 1 or 0, plan_out[tile] = 1 for a departing tile that is
//     not all zeros, else 0.
// (b) grid_store_plan_kernel, one workgroup per sensor: releases the found slots, ranks the flagged departing tiles in
//     tile order (a workgroup prefix sum over contiguous spans of tiles), ranks the slots by (effective stamp, index)
//     by counting, and writes plan_out[tile] = assigned slot + 1 or 0, the keys, the stamps, clock and counts.
// (c) grid_store_commit_kernel, tile form: a workgroup copies its own grid tile into its planned slot, then overwrites
//     the tile from scratch; tile 0 writes offset and origin.
// No launch reads what another workgroup of the same launch writes: (a) reads grid, store, keys, stamps, origin and
// offset and writes scratch, the plans, shift and scrolled; (b) reads the plans, stamps, clock, offset and
// shift and writes plan_out, keys, stamps, clock and counts, one workgroup per sensor; (c) reads shift, plan_out, grid (its own tile)
// and scratch and writes store, grid, offset and origin.  A slot read in (a) and rewritten in (c) is two launches
// apart.  Integers and bitwise copies only, no atomics: the same bits in every run, at every batch position and in a
// replay.  A step without a scroll costs the scalar loads and one exit per workgroup, three times.
#include "pof_grid.h"
#include "pof_sensor.h"

namespace {

using namespace pof_grid;

constexpr int kMaxSlots = 1024;
constexpr int kWaves = kCellThreads / 64;

struct GridStoreArgs {
    ScrollArgs s;
    int slots;
    int16_t *store;
    int32_t *store_key, *store_stamp, *clock, *plan_in, *plan_out, *counts;
};

// where the thread's run of a pass starts in slot j of sensor b: a [B][S][64][64] array, 16-byte aligned
__device__ __forceinline__ long long slot_run(const TileThread &me, int slots, int j, int pass)
{
    return (((long long)me.b * slots + j) * kTile + pass + me.ly0) * kTile + me.lx0;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ unsigned wave_or(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kCellThreads) void grid_store_stage_kernel(GridStoreArgs g, int tiles_x, int tiles)
{
    __shared__ int s_part[2][kWaves];
    const ScrollArgs &a = g.s;
    const int H = a.H, W = a.W, tid = threadIdx.x, S = g.slots;
    const TileThread me(tiles_x, tiles);
    const int b = me.b;
    int sx, sy;
    scroll_shift(a, b, sx, sy);
    if (me.tile == 0 && tid == 0) scroll_write_shift(a, b, sx, sy);
    if ((sx | sy) == 0) return;

    // the tile as a destination
    int ux, uy;
    const bool inside = scroll_source(me, tiles_x, tiles, sx, sy, ux, uy);
    int found = kMaxSlots;                                                     // the lowest slot that holds the tile
    if (!inside) {
        const int kx = a.offset[2 * b] + sx + me.tx, ky = a.offset[2 * b + 1] + sy + me.ty;
        const int32_t *key = g.store_key + 2 * (long long)b * S, *stamp = g.store_stamp + (long long)b * S;
        for (int j = tid; j < S; j += kCellThreads)
            if (stamp[j] != 0 && key[2 * j] == kx && key[2 * j + 1] == ky) found = min(found, j);
        found = wave_min(found);
        if ((tid & 63) == 0) s_part[0][tid >> 6] = found;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) found = min(found, s_part[0][w]);
    }
    for (int pass = 0; pass < kTile; pass += kRowsPerPass) {
        uint4 cells = make_uint4(0u, 0u, 0u, 0u);                              // unknown
        if (inside) cells = *reinterpret_cast<const uint4 *>(a.grid + me.run(H, W, ux, uy, pass));
        else if (found < kMaxSlots) cells = *reinterpret_cast<const uint4 *>(g.store + slot_run(me, S, found, pass));
        *reinterpret_cast<uint4 *>(a.scratch + me.run(H, W, me.tx, me.ty, pass)) = cells;
    }

    // the tile as a source: it departs when its destination lies outside the window
    const long long dx = (long long)me.tx - sx, dy = (long long)me.ty - sy;
    const bool departs = !(dx >= 0 && dx < tiles_x && dy >= 0 && dy < tiles / tiles_x);
    unsigned any = 0u;
    if (departs) {
        for (int pass = 0; pass < kTile; pass += kRowsPerPass) {
            const uint4 c = *reinterpret_cast<const uint4 *>(a.grid + me.run(H, W, me.tx, me.ty, pass));
            any |= c.x | c.y | c.z | c.w;
        }
        any = wave_or(any);
        if ((tid & 63) == 0) s_part[1][tid >> 6] = (int)any;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) any |= (unsigned)s_part[1][w];
    }
    if (tid == 0) {
        const long long at = (long long)b * tiles + me.tile;
        g.plan_in[at] = !inside && found < kMaxSlots ? found + 1 : 0;
        g.plan_out[at] = any != 0u ? 1 : 0;
    }
}

// Thread t owns the tiles [t * per, (t + 1) * per) of the sensor, so thread order is tile order, and the slots
// t, t + THREADS, ...: at most 8 of either a thread with 64 threads (up to 512 tiles and slots), at most 2 with 512.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void grid_store_plan_kernel(GridStoreArgs g, int tiles_x, int tiles)
{
    __shared__ int s_stamp[kMaxSlots];                         // the effective stamps
    __shared__ int s_order[kMaxSlots];                         // s_order[r] = the r-th slot of the slot order
    __shared__ int s_part[THREADS / 64];
    const ScrollArgs &a = g.s;
    const int b = blockIdx.x, tid = threadIdx.x, S = g.slots;
    int32_t *counts = g.counts + 4 * b;
    const int sx = a.shift[2 * b], sy = a.shift[2 * b + 1];
    if ((sx | sy) == 0) {
        if (tid < 4) counts[tid] = 0;
        return;
    }
    const int ox = a.offset[2 * b], oy = a.offset[2 * b + 1], now = g.clock[b] + 1;
    int32_t *key = g.store_key + 2 * (long long)b * S, *stamp = g.store_stamp + (long long)b * S;
    int32_t *plan_in = g.plan_in + (long long)b * tiles, *plan_out = g.plan_out + (long long)b * tiles;

    for (int j = tid; j < S; j += THREADS) s_stamp[j] = stamp[j];
    pof_lds_order<THREADS>();
    // release: a found slot is free again; two tiles have two keys, so no slot is found twice
    const int per = (tiles + THREADS - 1) / THREADS, t0 = min(tid * per, tiles), t1 = min(t0 + per, tiles);
    int restored = 0, leaving = 0;
    for (int t = t0; t < t1; ++t) {
        const int j = plan_in[t];
        if (j != 0) s_stamp[j - 1] = 0, ++restored;
        leaving += plan_out[t];
    }
    int n_leaving, n_restored;
    int rank = pof_sensor::group_exclusive<THREADS>(leaving, s_part, n_leaving);
    pof_sensor::group_exclusive<THREADS>(restored, s_part, n_restored);
    pof_lds_order<THREADS>();

    // the slot order by counting: the rank of slot j is the number of slots in front of it
    const int stored = min(n_leaving, S);
    int evicted = 0;
    for (int j = tid; j < S; j += THREADS) {
        const int e = s_stamp[j];
        int r = 0;
        for (int i = 0; i < S; ++i) {
            const int f = s_stamp[i];
            r += (f < e || (f == e && i < j)) ? 1 : 0;
        }
        s_order[r] = j;
        if (r < stored) {
            stamp[j] = now;
            evicted += e != 0 ? 1 : 0;
        } else {
            stamp[j] = e;                                      // a released slot that nothing took ends free
        }
    }
    int n_evicted;
    pof_sensor::group_exclusive<THREADS>(evicted, s_part, n_evicted);
    pof_lds_order<THREADS>();

    // the r-th flagged departing tile takes the r-th slot of the order
    for (int t = t0; t < t1; ++t) {
        int slot = 0;
        if (plan_out[t] != 0) {
            if (rank < S) {
                const int j = s_order[rank];
                key[2 * j] = ox + t % tiles_x;
                key[2 * j + 1] = oy + t / tiles_x;
                slot = j + 1;
            }
            ++rank;
        }
        plan_out[t] = slot;
    }
    if (tid == 0) {
        g.clock[b] = now;
        counts[0] = n_restored, counts[1] = stored, counts[2] = n_evicted, counts[3] = n_leaving - stored;
    }
}

__global__ __launch_bounds__(kCellThreads) void grid_store_commit_kernel(GridStoreArgs g, int tiles_x, int tiles)
{
    const ScrollArgs &a = g.s;
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const TileThread me(tiles_x, tiles);
    const int b = me.b;
    const int sx = a.shift[2 * b], sy = a.shift[2 * b + 1];
    if ((sx | sy) == 0) return;

    if (me.tile == 0 && tid == 0) scroll_write_origin(a, b, sx, sy);
    const int slot = g.plan_out[(long long)b * tiles + me.tile] - 1;
    for (int pass = 0; pass < kTile; pass += kRowsPerPass) {
        const long long at = me.run(H, W, me.tx, me.ty, pass);
        // the thread's own cells leave for the store before it overwrites them
        if (slot >= 0) *reinterpret_cast<uint4 *>(g.store + slot_run(me, g.slots, slot, pass)) = *reinterpret_cast<const uint4 *>(a.grid + at);
        *reinterpret_cast<uint4 *>(a.grid + at) = *reinterpret_cast<const uint4 *>(a.scratch + at);
    }
}

}  // namespace

extern "C" int pof_grid_scroll_store(const double *trans, double res, int margin, int slots, int B, int H, int W,
                                     int16_t *grid, double *origin, const double *base, int32_t *offset,
                                     int16_t *scratch, int16_t *store, int32_t *store_key, int32_t *store_stamp,
                                     int32_t *clock, int32_t *plan_in, int32_t *plan_out, int32_t *shift,
                                     uint8_t *scrolled, int32_t *counts, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    GridStoreArgs g;
    g.s = {trans, res, margin, H, W, grid, origin, base, offset, scratch, shift, scrolled};
    g.slots = slots; g.store = store; g.store_key = store_key; g.store_stamp = store_stamp; g.clock = clock;
    g.plan_in = plan_in; g.plan_out = plan_out; g.counts = counts;
    if (!store || !store_key || !store_stamp || !clock || !plan_in || !plan_out || !counts) return POF_E_BADARG;
    if (slots < 1 || slots > kMaxSlots) return POF_E_BADARG;
    const int refused = scroll_check(g.s, B);
    if (refused != POF_OK) return refused;
    if (reinterpret_cast<uintptr_t>(store) % 16) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    const Tiles tiles(H, W);
    grid_store_stage_kernel<<<B * tiles.all, kCellThreads, 0, pof_stream(stream)>>>(g, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    const int entries = tiles.all > slots ? tiles.all : slots;                 // <= 1024: picks the launch form
    POF_LAUNCH_PER_SENSOR(grid_store_plan_kernel, entries, B, stream, g, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    grid_store_commit_kernel<<<B * tiles.all, kCellThreads, 0, pof_stream(stream)>>>(g, tiles.x, tiles.all);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
