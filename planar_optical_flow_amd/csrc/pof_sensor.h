// What the per-scan stages behind the detector trunk share: one workgroup per sensor.  person_flow (N5), ego_motion (N6),
// pof_icp.h (N8-N10), person_motion (N11), the points launch of grid_map (N12), track_map (N15), the counts launch of
// grid_cast (N16), novel_segments (N17) and merge_detections (N18); grid_match (N13) and grid_cast's walk take gate, pose and hit rule only.
//
// Workgroup b owns sensor b.  Thread t holds the entries t, t + THREADS, ... of the sensor -- points, or detection
// rows -- in kSlots register slots: slot c of thread t is entry t + THREADS * c, so a load or store over t is coalesced
// and entry k belongs to thread k % THREADS, slot k / THREADS.  Two launch forms, chosen by the launcher from N alone:
//   N <= kWaveMaxN  (512):  THREADS = 64, one wave; its LDS traffic is ordered without a barrier (pof_lds_order);
//   N <= kGroupMaxN (4096): THREADS = kGroupThreads (512), workgroup barriers.  Beyond it a launcher returns
//                           POF_E_SHAPE; this is also the limit of pof_nms_predicted_center.
// A stage that walks the points of a scan stages them in LDS in chunks of kChunk.
//
// FIXED ORDER.  Every float64 sum has one order of additions: a thread adds its slots in slot order, sums over the
// workgroup meet in group_sum (pof_common.h), sums per detection row are added by the row's owning lane alone in
// ascending point index (row_sums).  No floating-point atomics, and with -ffp-contract=off no FMA that is not written
// out: the same bits in every run, at every batch position and in a graph replay, as the NumPy restatements need.
#pragma once
#include "pof_common.h"

namespace pof_sensor {

constexpr int kSlots = 8;                  // entries per thread
constexpr int kWaveMaxN = 64 * kSlots;
constexpr int kGroupThreads = 512;
constexpr int kGroupMaxN = kGroupThreads * kSlots;
constexpr int kChunk = 512;                // points staged in LDS at a time

// The two launch forms of a kernel template `kernel<THREADS>`, one workgroup per sensor on the stream.  A macro: the
// kernel is a template name.
#define POF_LAUNCH_PER_SENSOR(kernel, N, B, stream, ...)                                                           \
    do {                                                                                                           \
        if ((N) <= pof_sensor::kWaveMaxN) kernel<64><<<B, 64, 0, pof_stream(stream)>>>(__VA_ARGS__);               \
        else kernel<pof_sensor::kGroupThreads><<<B, pof_sensor::kGroupThreads, 0, pof_stream(stream)>>>(__VA_ARGS__); \
    } while (0)

// a count inside [0, N], one value for the workgroup: loop bounds and tests on it are scalar
__device__ __forceinline__ int clamped_count(int nd, int N)
{
    nd = __builtin_amdgcn_readfirstlane(nd);
    return nd < 0 ? 0 : (nd > N ? N : nd);
}

__device__ __forceinline__ int clamped_num_det(const int32_t *num_det, int b, int N) { return clamped_count(num_det[b], N); }

// The NMS's result as a gate on the points of a scan: point i belongs to detection row instance_mask - 1 when that is
// in [0, nd), nd = num(b, N), and to a person when the row's score reaches cls_thresh (pof_person_flow's det_valid).
// `row` = b * N.  A null instance_mask gates nothing.  A kernel that needs row and person loads the id once (id_of).
struct NmsGate {
    const int32_t *instance_mask, *num_det;
    const double *det_cls;
    double cls_thresh;

    // only the load is behind the test: the wait for it stays where nd is first used
    __device__ __forceinline__ int num(int b, int N) const { return clamped_count(instance_mask ? num_det[b] : 0, N); }

    __device__ __forceinline__ int id_of(long long row, int i) const { return instance_mask ? instance_mask[row + i] : 0; }

    // the detection row of a point with this id, or -1
    __device__ __forceinline__ int row_of(int id, int nd) const { return id >= 1 && id <= nd ? id - 1 : -1; }

    __device__ __forceinline__ bool id_is_person(long long row, int id, int nd) const
    {
        return id >= 1 && id <= nd && det_cls[row + id - 1] >= cls_thresh;
    }

    __device__ __forceinline__ bool is_person(long long row, int i, int nd) const
    {
        if (!instance_mask) return false;
        const int id = instance_mask[row + i];
        return id_is_person(row, id, nd);
    }
};

// the NMS results come together or not at all; a launcher answers POF_E_BADARG without it
inline bool nms_gate_ok(const int32_t *instance_mask, const int32_t *num_det, const double *det_cls)
{
    const int given = (instance_mask != nullptr) + (num_det != nullptr) + (det_cls != nullptr);
    return !(given != 0 && given != 3);
}

// a beam with an endpoint the map stages use: a NaN, an infinity, 0 and whatever reaches max_range have none
__device__ __forceinline__ bool is_hit(double r, double max_range) { return isfinite(r) && r > 0.0 && r < max_range; }

// The pose terms of sensor b (pof_write_pose_terms): rot[b] row-major in float, trans[b]; the ABI's two expressions.
struct SensorPose {
    float r00, r01, r10, r11;
    double tx, ty;

    __device__ __forceinline__ SensorPose(const float *rot, const double *trans, int b)
    {
        const float *R = rot + 4 * (long long)b;
        r00 = R[0], r01 = R[1], r10 = R[2], r11 = R[3];
        tx = trans[2 * b], ty = trans[2 * b + 1];
    }

    // a direction in the sensor frame to the world frame: two roundings per product and sum, no fma
    __device__ __forceinline__ void rotate(double px, double py, double &wx, double &wy) const
    {
        wx = (double)r00 * px + (double)r01 * py, wy = (double)r10 * px + (double)r11 * py;
    }

    // a difference of world points to the sensor frame: the transpose
    __device__ __forceinline__ void to_sensor(double dx, double dy, double &sx, double &sy) const
    {
        sx = (double)r00 * dx + (double)r10 * dy, sy = (double)r01 * dx + (double)r11 * dy;
    }

    // a scan point p = r (cos, sin)
    __device__ __forceinline__ void point_to_world(double px, double py, double &wx, double &wy) const
    {
        rotate(px, py, wx, wy);
        wx += tx, wy += ty;
    }

    // a detection centre d (det_xy_world): the only fma of these stages
    __device__ __forceinline__ void det_to_world(double d0, double d1, double &ox, double &oy) const
    {
        ox = fma(d1, (double)r01, d0 * (double)r00) + tx;
        oy = fma(d1, (double)r11, d0 * (double)r10) + ty;
    }
};

// exclusive prefix of v over the workgroup in thread order, total = the sum; s_part: THREADS / 64 ints
template <int THREADS>
__device__ __forceinline__ int group_exclusive(int v, int *s_part, int &total)
{
    const int lane = threadIdx.x & 63;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (THREADS == 64) {
        total = __shfl(incl, 63, 64);
        return incl - v;
    }
    constexpr int kWaves = THREADS / 64;
    const int wave = threadIdx.x >> 6;
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int p = s_part[w];
        if (w < wave) before += p;
        sum += p;
    }
    __syncthreads();                                           // the next call writes s_part
    total = sum;
    return before + incl - v;
}

// An empty statement the compiler may not speculate: a block that holds it stays behind its branch.  Without it the
// wave-uniform tests on the register slot become selects and the float64 work of all kSlots slots runs for every entry.
__device__ __forceinline__ void keep_branch() { asm volatile(""); }

// the value lane l of the wave holds; l is wave-uniform
__device__ __forceinline__ double lane_value(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// Sums per detection row over n <= kChunk staged points, point order kept: s_id[j] is the instance id of staged point
// j (row + 1; outside [1, nd]: nobody's) and s_v[k][j] its K values.  Every wave steps through all staged points in
// ascending j and only the row's owner -- thread row % THREADS, slot row / THREADS -- adds, so a row's sum is
// sequential in point order whatever the other waves do.  A wave takes 64 points into registers at once, lane l point
// j0 + l, and walks the set bits of a ballot in ascending l; id and values leave the lane by v_readlane, so they are
// wave-uniform: one LDS read per 64 points, a scalar branch per slot, and a wave that does not own the row skips it.
// Lanes at or beyond n read what LDS holds (inside the array: STRIDE >= kChunk); the ballot leaves them out.  The
// caller orders the staging in front of the call and the next chunk's behind it (pof_lds_order).
template <int THREADS, int K, int STRIDE>
__device__ __forceinline__ void row_sums(const int *s_id, const double (&s_v)[K][STRIDE], int n, int nd,
                                         double (&acc)[kSlots][K], int (&cnt)[kSlots])
{
    static_assert(STRIDE >= kChunk, "a wave reads whole groups of 64 staged points");
    const int tid = threadIdx.x, lane = tid & 63, my_wave = tid >> 6;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int mine = j0 + lane;                            // < kChunk: j0 is a multiple of 64 below it
        const int id = mine < n ? s_id[mine] : 0;
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = s_v[k][mine];
        unsigned long long todo = __ballot(id >= 1 && id <= nd);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int row = __builtin_amdgcn_readlane(id, l) - 1;
            const int owner = row % THREADS, slot = row / THREADS;
            if ((owner >> 6) != my_wave) continue;
            double u[K];
#pragma unroll
            for (int k = 0; k < K; ++k) u[k] = lane_value(v[k], l);
#pragma unroll
            for (int c = 0; c < kSlots; ++c) {
                if (c == slot) {                               // wave-uniform: a scalar branch
                    keep_branch();
                    if (tid == owner) {
#pragma unroll
                        for (int k = 0; k < K; ++k) acc[c][k] += u[k];
                        ++cnt[c];
                    }
                }
            }
        }
    }
}

}  // namespace pof_sensor
