// N7: person tracks over the per-person flow, one launch per batch, one wave per sensor.
//
// The detections of a scan (pof_person_flow's det_xy_world / det_flow / det_valid, the NMS's num_det / instance_mask)
// are associated with M = max_tracks slots of persistent state by a gated greedy global nearest neighbour, and every
// track is a constant-velocity Kalman filter whose time step is one scan.  All noises are isotropic, so one 2x2
// covariance block (a, b, c) = (var p, cov p v, var v) serves both axes.  One step (include/pof_abi.h has the contract):
//   1. predict live slots:  p += v;  a <- (a + b) + (b + c), b <- b + c, c <- c + q;  age += 1
//   2. candidates: rows k < num_det with det_valid != 0 and a finite centre, in row order
//   3. cost(t, k) = dx dx + dy dy, taking part while cost <= gate^2
//   4. repeatedly the smallest cost among unassigned slots and candidates; ties: lower slot, then lower row
//   5. matched: position update, then (finite flow) velocity update; hits += 1, misses = 0
//   6. unmatched: misses += 1, beyond max_misses the slot is zeroed
//   7. births: unmatched candidates in row order into the lowest free slots, id = next_id++; none free: dropped += 1
//   8. track_det / track_confirmed / det_track / point_track / dropped
//
// Shape: lane l owns the slots l, l + 64, ... (J = 1 for M <= 64, else 4) in registers.  The candidates are compacted
// by ballot / popcount into LDS: their rows, and their centres in chunks of kChunk (every scan of practice is one
// chunk, staged once).  A taken candidate's staged centre becomes NaN, so the cost loop needs no flag: a NaN cost is
// never inside the gate.  Every slot caches its best candidate and looks again only when that candidate was taken; a
// candidate that stays is still the slot's best, because the costs of a round do not change.  The round's winner is a
// __shfl_xor butterfly over (cost, slot): both lanes of a pair make the same comparison and slots are distinct, so all
// 64 lanes end with the same winner.  The births of step 7 are sequential in the statement but independent: the r-th
// unmatched candidate takes the r-th free slot and the id next_id + r.  No atomics, plain float64 multiplies and adds
// in the stated order (-ffp-contract=off): the same bits in every run, at every batch position and in a graph replay.
// Candidate cap: every row may be a candidate, i.e. N <= 4096.  Latency bound like the launches it follows.
#include <climits>
#include <cmath>

#include "pof_sensor.h"                                         // clamped_num_det only: the slot scheme here is its own

namespace {

constexpr int kMaxTracks = 256;
constexpr int kMaxN = 4096;        // the limit of pof_nms_predicted_center; also the candidate cap
constexpr int kChunk = 1024;       // candidate centres staged in LDS at a time

struct TrackArgs {
    const double *det_xy_world, *det_flow;
    const uint8_t *det_valid;
    const int32_t *num_det, *instance_mask;
    int N, M;
    int32_t *track_id;
    double *track_state, *track_cov;
    int32_t *track_hits, *track_misses, *track_age, *next_id;
    int32_t *track_det;
    uint8_t *track_confirmed;
    int32_t *det_track, *point_track, *dropped;
    double gate, q, r_pos, r_vel, v0_var;
    int max_misses, min_hits;
};

template <int J>
__global__ __launch_bounds__(64) void track_update_kernel(TrackArgs a)
{
    __shared__ double s_zx[kChunk], s_zy[kChunk];              // centres of the staged chunk; NaN once taken
    __shared__ int32_t s_dt[kMaxN];                            // det_track of this sensor
    __shared__ uint16_t s_row[kMaxN];                          // candidate -> detection row
    __shared__ uint8_t s_taken[kMaxN];
    __shared__ uint16_t s_birth[kMaxTracks];                   // the first unmatched candidates, in row order
    const int N = a.N, M = a.M, b = blockIdx.x, lane = threadIdx.x;
    const long long drow = (long long)b * N, trow = (long long)b * M;
    const unsigned long long below = (1ull << lane) - 1ull;
    const double qnan = __builtin_nan(""), inf = __builtin_inf();
    const double gate2 = a.gate * a.gate;
    const int nd = pof_sensor::clamped_num_det(a.num_det, b, N);
    const int first_id = a.next_id[b];

    int id[J], hits[J], misses[J], age[J], match[J], bi[J];
    double x[J], y[J], vx[J], vy[J], ca[J], cb[J], cc[J], bc[J];
    bool live[J], stale[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int t = lane + 64 * j;
        id[j] = hits[j] = misses[j] = age[j] = 0;
        x[j] = y[j] = vx[j] = vy[j] = ca[j] = cb[j] = cc[j] = 0.0;
        if (t < M) {
            id[j] = a.track_id[trow + t];
            hits[j] = a.track_hits[trow + t];
            misses[j] = a.track_misses[trow + t];
            age[j] = a.track_age[trow + t];
            x[j] = a.track_state[4 * (trow + t)];
            y[j] = a.track_state[4 * (trow + t) + 1];
            vx[j] = a.track_state[4 * (trow + t) + 2];
            vy[j] = a.track_state[4 * (trow + t) + 3];
            ca[j] = a.track_cov[3 * (trow + t)];
            cb[j] = a.track_cov[3 * (trow + t) + 1];
            cc[j] = a.track_cov[3 * (trow + t) + 2];
        }
        live[j] = stale[j] = id[j] != 0;
        match[j] = bi[j] = -1;
        bc[j] = inf;
        if (live[j]) {                                         // 1. predict
            x[j] += vx[j];
            y[j] += vy[j];
            const double a0 = ca[j], b0 = cb[j], c0 = cc[j];
            ca[j] = (a0 + b0) + (b0 + c0);
            cb[j] = b0 + c0;
            cc[j] = c0 + a.q;
            age[j] += 1;
        }
    }

    // 2. candidates, compacted in row order
    int C = 0;
    for (int base = 0; base < nd; base += 64) {
        const int k = base + lane;
        bool ok = false;
        if (k < nd && a.det_valid[drow + k])
            ok = isfinite(a.det_xy_world[2 * (drow + k)]) && isfinite(a.det_xy_world[2 * (drow + k) + 1]);
        const unsigned long long mask = __ballot(ok);
        if (ok) {
            const int c = C + __popcll(mask & below);
            s_row[c] = (uint16_t)k;
            s_taken[c] = 0;
        }
        C += __popcll(mask);
    }
    __syncthreads();

    // 3.-5. greedy global nearest neighbour
    int staged = -1;                                           // first candidate of the chunk held in s_zx / s_zy
    for (;;) {
        bool any_stale = false;
#pragma unroll
        for (int j = 0; j < J; ++j) any_stale = any_stale || stale[j];
        if (__ballot(any_stale) != 0ull) {                     // uniform: all lanes stage, the stale slots look
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (stale[j]) {
                    bc[j] = inf;
                    bi[j] = -1;
                }
            }
            for (int base = 0; base < C; base += kChunk) {
                const int n = C - base < kChunk ? C - base : kChunk;
                if (staged != base) {
                    __syncthreads();                           // everyone has left the chunk that is replaced
                    for (int i = lane; i < n; i += 64) {
                        const long long p = drow + s_row[base + i];
                        const bool taken = s_taken[base + i] != 0;
                        s_zx[i] = taken ? qnan : a.det_xy_world[2 * p];
                        s_zy[i] = taken ? qnan : a.det_xy_world[2 * p + 1];
                    }
                    staged = base;
                    __syncthreads();
                }
                for (int i = 0; i < n; ++i) {
                    const double zx = s_zx[i], zy = s_zy[i];   // one address for all lanes: a broadcast
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        if (stale[j]) {
                            const double dx = zx - x[j], dy = zy - y[j];
                            const double cost = dx * dx + dy * dy;
                            if (cost <= gate2 && cost < bc[j]) {   // strict: the lower row keeps a tie
                                bc[j] = cost;
                                bi[j] = base + i;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < J; ++j) stale[j] = false;
        }

        // this lane's best pair, then the wave's: smallest cost, then lowest slot
        double wc = inf;
        int ws = INT_MAX, wi = -1;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (live[j] && match[j] < 0 && bi[j] >= 0 && bc[j] < wc) {
                wc = bc[j];
                ws = lane + 64 * j;
                wi = bi[j];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double oc = __shfl_xor(wc, o, 64);
            const int os = __shfl_xor(ws, o, 64), oi = __shfl_xor(wi, o, 64);
            if (oc < wc || (oc == wc && os < ws)) {
                wc = oc;
                ws = os;
                wi = oi;
            }
        }
        if (wi < 0) break;                                     // uniform: no pair inside the gate is left

#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (ws == lane + 64 * j) {                         // 5. the owner of the winning slot
                const int k = s_row[wi];
                const long long p = drow + k;
                const double zx = a.det_xy_world[2 * p], zy = a.det_xy_world[2 * p + 1];
                const double fx = a.det_flow[2 * p], fy = a.det_flow[2 * p + 1];
                {
                    const double s = ca[j] + a.r_pos, k1 = ca[j] / s, k2 = cb[j] / s;
                    const double rx = zx - x[j], ry = zy - y[j];
                    x[j] += k1 * rx;
                    y[j] += k1 * ry;
                    vx[j] += k2 * rx;
                    vy[j] += k2 * ry;
                    const double a0 = ca[j], b0 = cb[j], c0 = cc[j];
                    ca[j] = a0 - k1 * a0;
                    cb[j] = b0 - k1 * b0;
                    cc[j] = c0 - k2 * b0;
                }
                if (isfinite(fx) && isfinite(fy)) {
                    const double s = cc[j] + a.r_vel, k1 = cb[j] / s, k2 = cc[j] / s;
                    const double rx = fx - vx[j], ry = fy - vy[j];
                    x[j] += k1 * rx;
                    y[j] += k1 * ry;
                    vx[j] += k2 * rx;
                    vy[j] += k2 * ry;
                    const double a0 = ca[j], b0 = cb[j], c0 = cc[j];
                    ca[j] = a0 - k1 * b0;
                    cb[j] = b0 - k1 * c0;
                    cc[j] = c0 - k2 * c0;
                }
                hits[j] += 1;
                misses[j] = 0;
                match[j] = k;
                s_taken[wi] = 1;
                if (wi >= staged && wi < staged + kChunk) s_zx[wi - staged] = s_zy[wi - staged] = qnan;
            }
        }
        __syncthreads();                                       // the next look sees the candidate gone
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (live[j] && match[j] < 0 && bi[j] == wi) stale[j] = true;
    }

    // 6. unmatched live slots
#pragma unroll
    for (int j = 0; j < J; ++j) {
        if (live[j] && match[j] < 0) {
            misses[j] += 1;
            if (misses[j] > a.max_misses) {
                id[j] = hits[j] = misses[j] = age[j] = 0;
                x[j] = y[j] = vx[j] = vy[j] = ca[j] = cb[j] = cc[j] = 0.0;
            }
        }
    }

    // 7. births: the r-th unmatched candidate takes the r-th free slot
    int n_free = 0, frank[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const bool is_free = lane + 64 * j < M && id[j] == 0;
        const unsigned long long mask = __ballot(is_free);
        frank[j] = is_free ? n_free + __popcll(mask & below) : -1;
        n_free += __popcll(mask);
    }
    int U = 0;
    for (int base = 0; base < C; base += 64) {
        const int c = base + lane;
        const bool un = c < C && s_taken[c] == 0;
        const unsigned long long mask = __ballot(un);
        const int r = U + __popcll(mask & below);
        if (un && r < kMaxTracks) s_birth[r] = (uint16_t)c;
        U += __popcll(mask);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) {
        if (frank[j] >= 0 && frank[j] < U) {                   // frank < n_free <= M <= kMaxTracks
            const int k = s_row[s_birth[frank[j]]];
            const long long p = drow + k;
            const double fx = a.det_flow[2 * p], fy = a.det_flow[2 * p + 1];
            const bool with_flow = isfinite(fx) && isfinite(fy);
            id[j] = first_id + frank[j];
            x[j] = a.det_xy_world[2 * p];
            y[j] = a.det_xy_world[2 * p + 1];
            vx[j] = with_flow ? fx : 0.0;
            vy[j] = with_flow ? fy : 0.0;
            ca[j] = a.r_pos;
            cb[j] = 0.0;
            cc[j] = with_flow ? a.r_vel : a.v0_var;
            hits[j] = 1;
            misses[j] = age[j] = 0;
            match[j] = k;
        }
    }
    const int births = U < n_free ? U : n_free;

    // 8. outputs and the state
    for (int i = lane; i < N; i += 64) s_dt[i] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int t = lane + 64 * j;
        if (t < M) {
            if (id[j] == 0) match[j] = -1;                     // a slot freed in step 6
            if (match[j] >= 0) s_dt[match[j]] = id[j];
            a.track_id[trow + t] = id[j];
            a.track_hits[trow + t] = hits[j];
            a.track_misses[trow + t] = misses[j];
            a.track_age[trow + t] = age[j];
            a.track_state[4 * (trow + t)] = x[j];
            a.track_state[4 * (trow + t) + 1] = y[j];
            a.track_state[4 * (trow + t) + 2] = vx[j];
            a.track_state[4 * (trow + t) + 3] = vy[j];
            a.track_cov[3 * (trow + t)] = ca[j];
            a.track_cov[3 * (trow + t) + 1] = cb[j];
            a.track_cov[3 * (trow + t) + 2] = cc[j];
            a.track_det[trow + t] = match[j];
            a.track_confirmed[trow + t] = id[j] != 0 && hits[j] >= a.min_hits ? 1 : 0;
        }
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
        const int inst = a.instance_mask[drow + i];
        a.det_track[drow + i] = s_dt[i];
        a.point_track[drow + i] = inst >= 1 && inst <= nd ? s_dt[inst - 1] : 0;
    }
    if (lane == 0) {
        a.next_id[b] = first_id + births;
        a.dropped[b] = U - births;
    }
}

}  // namespace

extern "C" int pof_track_update(const double *det_xy_world, const double *det_flow, const uint8_t *det_valid,
                                const int32_t *num_det, const int32_t *instance_mask, int B, int N, int max_tracks,
                                int32_t *track_id, double *track_state, double *track_cov, int32_t *track_hits,
                                int32_t *track_misses, int32_t *track_age, int32_t *next_id, int32_t *track_det,
                                uint8_t *track_confirmed, int32_t *det_track, int32_t *point_track, int32_t *dropped,
                                double gate, double q, double r_pos, double r_vel, double v0_var, int max_misses,
                                int min_hits, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!det_xy_world || !det_flow || !det_valid || !num_det || !instance_mask || !track_id || !track_state ||
        !track_cov || !track_hits || !track_misses || !track_age || !next_id || !track_det || !track_confirmed ||
        !det_track || !point_track || !dropped)
        return POF_E_BADARG;
    if (B < 0 || N < 1 || max_tracks < 1 || max_misses < 0) return POF_E_BADARG;
    if (!(gate >= 0.0) || !(q >= 0.0) || !(r_pos > 0.0) || !(r_vel > 0.0) || !(v0_var > 0.0)) return POF_E_BADARG;
    if (N > kMaxN || max_tracks > kMaxTracks) return POF_E_SHAPE;
    if (B == 0) return POF_OK;
    TrackArgs a;
    a.det_xy_world = det_xy_world; a.det_flow = det_flow; a.det_valid = det_valid; a.num_det = num_det;
    a.instance_mask = instance_mask; a.N = N; a.M = max_tracks; a.track_id = track_id; a.track_state = track_state;
    a.track_cov = track_cov; a.track_hits = track_hits; a.track_misses = track_misses; a.track_age = track_age;
    a.next_id = next_id; a.track_det = track_det; a.track_confirmed = track_confirmed; a.det_track = det_track;
    a.point_track = point_track; a.dropped = dropped; a.gate = gate; a.q = q; a.r_pos = r_pos; a.r_vel = r_vel;
    a.v0_var = v0_var; a.max_misses = max_misses; a.min_hits = min_hits;
    if (max_tracks <= 64)
        track_update_kernel<1><<<B, 64, 0, pof_stream(stream)>>>(a);
    else
        track_update_kernel<4><<<B, 64, 0, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
