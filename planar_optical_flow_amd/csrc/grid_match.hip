// N13: scan-to-grid matching, an exhaustive (correlative) search over whole-cell translations and a small table of
// rotations, scored with integers only against the int16 grid of N12.  One entry point, two launches on the caller's
// stream; include/pof_abi.h has the contract.
//
// (a) grid_match_scores_kernel, one workgroup of 256 threads per (sensor, rotation).  The N cells of the rotated scan are
//     staged once in LDS as a packed pair of int16 (g_x, g_y) -- the only float64 work of the launch, N points per
//     workgroup, by N12's point_cell arithmetic (SensorPose, then pof_grid.h's Cell) behind the rotation of the table
//     row.  Only points that vote and can reach the grid within R are staged: they are appended through an integer LDS
//     counter, so the walk below has no sentinel to test (their order differs from run to run; an integer sum has none).
//     The T T translations are then split over the threads together with the staged points: with S = max(1, 256 / (T T))
//     slices, work item w = slice (T T) + translation belongs to thread w % 256 and walks the staged points slice,
//     slice + S, ..., gathering int16 from the sensor's grid.  Neighbouring threads hold neighbouring dx of one slice,
//     so a wave's gathers for one point fall into one or two 128-byte lines of a grid row (and into a second pair where
//     the wave crosses a row of the search or a slice).  The slices meet in LDS with integer atomics.  At the defaults
//     (T T = 81, S = 3) 243 of the 256 threads work; at the largest search (T T = 1089) every thread owns 4 or 5
//     translations and walks all points.
// (b) grid_match_pick_kernel, one wave per sensor: every lane packs (score, inverted rank) of its candidates into one
//     64-bit key, the rank being (dx dx + dy dy, |kappa|, flat index) -- the tie rule, most significant first -- and
//     the wave reduces the keys with a max in a butterfly, so every lane ends with the same bits.  Lane 0 applies the
//     gates in int64 and writes the outputs, and with `moved` the pose and its terms (pof_write_pose_terms).
//
// No global atomics, integer sums only: the same bits in every run, at every batch position and in a replay.
#include <cmath>

#include "pof_grid.h"
#include "pof_sensor.h"

namespace {

using namespace pof_sensor;
using pof_grid::Cell;

constexpr int kScoreThreads = 256;
constexpr int kMaxReach = 16, kMaxRotations = 33;
constexpr int kMaxT = 2 * kMaxReach + 1;

struct GridMatchArgs {
    const float *ranges;
    const double *tab;
    NmsGate gate;
    double max_range;
    const int16_t *grid;
    const double *origin;
    double res;
    const double *rot_tab;
    int reach, rotations, min_points, min_score, min_gain, N, H, W;
    double *pose;
    float *rot;
    double *trans;
    int32_t *scores, *best, *score, *votes;
    uint8_t *ok, *moved;
    double *correction;
};

__global__ __launch_bounds__(kScoreThreads) void grid_match_scores_kernel(GridMatchArgs a)
{
    __shared__ int s_cell[kGroupMaxN];                         // (g_y << 16) | (g_x & 0xffff) of the staged points
    __shared__ int s_acc[kMaxT * kMaxT];
    __shared__ int s_staged, s_votes;
    const int N = a.N, H = a.H, W = a.W, R = a.reach, K = a.rotations, tid = threadIdx.x;
    const int T = 2 * R + 1, TT = T * T;
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const long long row = (long long)b * N;
    const int nd = a.gate.num(b, N);
    const SensorPose pose(a.rot, a.trans, b);
    const double ox = a.origin[2 * b], oy = a.origin[2 * b + 1];
    const double ck = a.rot_tab[3 * k + 1], sk = a.rot_tab[3 * k + 2];
    const int16_t *grid = a.grid + (long long)b * H * W;

    if (tid == 0) s_staged = s_votes = 0;
    for (int t = tid; t < TT; t += kScoreThreads) s_acc[t] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += kScoreThreads) {
        const double r = (double)a.ranges[row + i];
        if (!is_hit(r, a.max_range) || a.gate.is_person(row, i, nd)) continue;
        atomicAdd(&s_votes, 1);
        const double px = r * a.tab[N + 2 * i], py = r * a.tab[N + 2 * i + 1];
        double wx, wy;
        pose.point_to_world(ck * px - sk * py, sk * px + ck * py, wx, wy);
        const Cell g = Cell::of(wx, wy, ox, oy, a.res);
        if (g.within(R, H, W))
            s_cell[atomicAdd(&s_staged, 1)] = (int)((unsigned)(int)g.gy << 16 | ((unsigned)(int)g.gx & 0xffffu));
    }
    __syncthreads();
    const int n = s_staged;
    if (k == (K - 1) / 2 && tid == 0) a.votes[b] = s_votes;

    const int slices = TT < kScoreThreads ? kScoreThreads / TT : 1;
    for (int w = tid; w < slices * TT; w += kScoreThreads) {
        const int slice = w / TT, t = w - slice * TT;
        const int dy = t / T - R, dx = t - (t / T) * T - R;
        int acc = 0;
#pragma unroll 8
        for (int j = slice; j < n; j += slices) {
            const int c = s_cell[j];
            const int x = (int)(short)(c & 0xffff) + dx, y = (c >> 16) + dy;
            const bool inside = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
            const int v = (int)grid[inside ? y * W + x : 0];   // always a load inside the grid: no branch in the walk
            acc += inside ? v : 0;
        }
        atomicAdd(&s_acc[t], acc);
    }
    __syncthreads();
    int32_t *out = a.scores + ((long long)b * K + k) * TT;
    for (int t = tid; t < TT; t += kScoreThreads) out[t] = s_acc[t];
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
        const unsigned long long u = (unsigned long long)hi << 32 | lo;
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void grid_match_pick_kernel(GridMatchArgs a)
{
    const int R = a.reach, K = a.rotations, T = 2 * R + 1, TT = T * T, mid = (K - 1) / 2;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t *scores = a.scores + (long long)b * K * TT;
    // rank: 10 bits of dx dx + dy dy (<= 512), 5 of |kappa| (<= 16), 16 of the flat index (< 33 * 1089)
    unsigned long long key = 0ull;
    for (int f = lane; f < K * TT; f += 64) {
        const int k = f / TT, t = f - k * TT;
        const int dy = t / T - R, dx = t - (t / T) * T - R, kappa = k - mid;
        const unsigned rank = (unsigned)(dx * dx + dy * dy) << 21 | (unsigned)(kappa < 0 ? -kappa : kappa) << 16 | (unsigned)f;
        const unsigned biased = (unsigned)scores[f] ^ 0x80000000u;             // int32 order as unsigned order
        const unsigned long long mine = (unsigned long long)biased << 32 | (0x7fffffffu - rank);
        key = mine > key ? mine : key;
    }
    key = wave_max_u64(key);
    if (lane != 0) return;
    const int f = (int)((0x7fffffffu - (unsigned)key) & 0xffffu);
    const int best = (int)((unsigned)(key >> 32) ^ 0x80000000u);
    const int k = f / TT, t = f - k * TT;
    const int dy = t / T - R, dx = t - (t / T) * T - R;
    const int zero_at = mid * TT + R * T + R, zero = scores[zero_at];
    const long long V = (long long)a.votes[b];
    const bool ok = V >= (long long)a.min_points && (long long)best >= (long long)a.min_score * V;
    const bool moved = ok && f != zero_at && (long long)best - (long long)zero >= (long long)a.min_gain * V;
    a.best[3 * b] = k - mid;
    a.best[3 * b + 1] = dy;
    a.best[3 * b + 2] = dx;
    a.score[2 * b] = best;
    a.score[2 * b + 1] = zero;
    a.ok[b] = ok ? 1 : 0;
    a.moved[b] = moved ? 1 : 0;
    double cx = 0.0, cy = 0.0, ct = 0.0;
    if (moved) {
        cx = (double)dx * a.res;
        cy = (double)dy * a.res;
        ct = a.rot_tab[3 * k];
        const double x = a.pose[3 * b] + cx, y = a.pose[3 * b + 1] + cy, phi = a.pose[3 * b + 2] + ct;
        a.pose[3 * b] = x;
        a.pose[3 * b + 1] = y;
        a.pose[3 * b + 2] = phi;
        pof_write_pose_terms(b, x, y, phi, 0.0, 0.0, a.rot, a.trans, nullptr);
    }
    a.correction[3 * b] = cx;
    a.correction[3 * b + 1] = cy;
    a.correction[3 * b + 2] = ct;
}

}  // namespace

extern "C" int pof_grid_match(const float *ranges, const double *tab, const int32_t *instance_mask,
                              const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range,
                              const int16_t *grid, const double *origin, double res, const double *rot_tab, int reach,
                              int rotations, int min_points, int min_score, int min_gain, int B, int N, int H, int W,
                              double *pose, float *rot, double *trans, int32_t *scores, int32_t *best, int32_t *score,
                              int32_t *votes, uint8_t *ok, uint8_t *moved, double *correction, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges || !tab || !grid || !origin || !rot_tab || !pose || !rot || !trans || !scores || !best || !score ||
        !votes || !ok || !moved || !correction)
        return POF_E_BADARG;
    if (!nms_gate_ok(instance_mask, num_det, det_cls)) return POF_E_BADARG;
    if (!(res > 0.0) || !(max_range > 0.0) || reach < 0 || reach > kMaxReach || rotations < 1 ||
        rotations > kMaxRotations || rotations % 2 == 0 || min_points < 0 || min_score < 0 || min_gain < 0 || B < 0 ||
        N < 1)
        return POF_E_BADARG;
    if (N > kGroupMaxN || !pof_grid::shape_ok(H, W)) return POF_E_SHAPE;
    if ((long long)B * rotations > 0x7fffffffLL) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    GridMatchArgs a;
    a.ranges = ranges; a.tab = tab; a.gate = {instance_mask, num_det, det_cls, cls_thresh}; a.max_range = max_range;
    a.grid = grid; a.origin = origin; a.res = res; a.rot_tab = rot_tab; a.reach = reach; a.rotations = rotations;
    a.min_points = min_points; a.min_score = min_score; a.min_gain = min_gain; a.N = N; a.H = H; a.W = W;
    a.pose = pose; a.rot = rot; a.trans = trans; a.scores = scores; a.best = best; a.score = score; a.votes = votes;
    a.ok = ok; a.moved = moved; a.correction = correction;
    grid_match_scores_kernel<<<B * rotations, kScoreThreads, 0, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    grid_match_pick_kernel<<<B, 64, 0, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
