// N9: keyframe scan matching -- the current scan is matched against a reference scan (the keyframe) that stays fixed
// until the sensor has moved away from it, and the pose is key_pose o (theta, u): no fit error accumulates while one
// keyframe is held.  One launch per batch, one sensor per workgroup; the keyframe, its pose, the last good match, the
// bookkeeping and the pose are persistent state updated in place, so a captured step stays one linear chain with no
// host decision.  The reference has no scan matcher: the specification is the N9 comment of include/pof_abi.h,
// restated in float64 NumPy by tests/test_keyframe.py (keyframe_oracle).  This file states only what differs from
// pof_scan_match (scan_match.hip), whose gate, line partner, normal, residual, Huber weight, sums, solve, composition
// and stop rule it repeats operation for operation.
//
// Window centre.  The keyframe may be tens of beams away from the current scan in every direction, so the window of a
// point is centred on the beam its transformed position falls on:
//   q = R(theta) p + u,  mid = (int)clamp(rint((atan2(q_y, q_x) - tab[0]) / dphi), -N, 2N)
// (0 when dphi == 0, -N for a NaN), searched over [mid - W, mid + W] n [0, N) upwards with a strict <.  No wrap-around.
//
// One step: see the header.  A workgroup reads its key_ranges row only while staging (before the first barrier) and
// every thread writes only the beams it staged itself, after the last correspondence pass: the replacement is in
// place.  The scalar state of a sensor is read by every thread before the first barrier and written by thread 0 at the
// end.
//
// As scan_match.hip: the keyframe's vertices staged once in LDS (two doubles per beam, NaN = not valid), kSlots points
// per thread in registers, twelve sums in a FIXED ORDER through group_sum (plus one, before the loop, that counts the
// current points that vote), no atomics and with -ffp-contract=off no FMA, every lane solves redundantly, the loop
// exit is uniform.  N <= 512: one wave per sensor;  N <= 4096: 512 threads per sensor.
#include <cmath>

#include "pof_common.h"

namespace {

constexpr int kSlots = 8;          // points per thread
constexpr int kWaveMaxN = 64 * kSlots;
constexpr int kGroupThreads = 512;
constexpr int kGroupMaxN = kGroupThreads * kSlots;
constexpr int kMaxIters = 32;
constexpr int kMaxWindow = 64;
constexpr int kSums = 12;

struct KeyframeArgs {
    const float *ranges_cur;
    const double *tab;
    const int32_t *instance_mask, *num_det;
    const double *det_cls;
    double cls_thresh, max_range, gate2, gap2, huber_delta, eps_theta, eps_u, min_pivot;
    double key_rot, key_dist2, min_share;
    int window, iters, max_misses, N;
    float *key_ranges;
    double *key_pose, *key_rel;
    uint8_t *key_valid;
    int32_t *key_age, *key_misses;
    double *pose;
    double *motion;
    int32_t *count;
    double *rms;
    uint8_t *ok;
    int32_t *iters_used;
    double *obs;
    uint8_t *key_replaced;
    int32_t *corr;
    double *flow_residual;
    float *rot;
    double *trans, *flow_trans;
};

// Sum of K values over the workgroup, the same bits in every thread (as in scan_match.hip).  `part` is [K][8]
// doubles of LDS (unused by the one-wave form).
template <int THREADS, int K>
__device__ __forceinline__ void group_sum(double (&v)[K], double *part)
{
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_f64(v[k]);
    if (THREADS > 64) {
        constexpr int kWaves = THREADS / 64;
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) part[k * kWaves + wave] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = part[k * kWaves];
#pragma unroll
            for (int j = 1; j < kWaves; ++j) s += part[k * kWaves + j];
            v[k] = s;
        }
        __syncthreads();                                       // the next sum overwrites the partials
    }
}

struct Rel {
    double th, ux, uy, c, s;
};

struct Match {
    int j;
    double qx, qy, dx, dy, nx, ny;
};

// the beam the point q falls on; phi0 = tab[0]
__device__ __forceinline__ int beam_of(double qx, double qy, double phi0, double dphi, int N)
{
    if (dphi == 0.0) return 0;
    double t = rint((atan2(qy, qx) - phi0) / dphi);
    if (!(t >= (double)-N)) t = (double)-N;
    if (!(t <= (double)(2 * N))) t = (double)(2 * N);
    return (int)t;
}

// the correspondence of the point (px, py); ax / ay: the staged vertices, every index read lies in [0, N)
__device__ __forceinline__ bool correspond(const double *ax, const double *ay, int N, int W, double gate2, double gap2,
                                           double phi0, double dphi, const Rel &m, double px, double py, Match &o)
{
    o.qx = (m.c * px - m.s * py) + m.ux;
    o.qy = (m.s * px + m.c * py) + m.uy;
    const int mid = beam_of(o.qx, o.qy, phi0, dphi, N);        // in [-N, 2N], N <= 4096: no overflow
    const int lo = mid - W < 0 ? 0 : mid - W;
    const int hi = mid + W > N - 1 ? N - 1 : mid + W;
    int best = -1;
    double bd = __builtin_inf();
    for (int j = lo; j <= hi; ++j) {
        const double dx = o.qx - ax[j], dy = o.qy - ay[j];
        const double d2 = dx * dx + dy * dy;                   // NaN for a vertex that is not valid: never <
        if (d2 < bd) {
            bd = d2;
            best = j;
        }
    }
    if (best < 0 || !(bd <= gate2)) return false;
    const double jx = ax[best], jy = ay[best];
    int k = -1;
    double ex = 0.0, ey = 0.0, l2 = 0.0, kd = 0.0;
#pragma unroll
    for (int side = -1; side <= 1; side += 2) {
        const int kk = best + side;
        if (kk < 0 || kk >= N) continue;
        const double kx = ax[kk], ky = ay[kk];
        const double fx = kx - jx, fy = ky - jy;
        const double f2 = fx * fx + fy * fy;
        if (!(f2 > 0.0 && f2 <= gap2)) continue;               // NaN: not valid
        const double gx = o.qx - kx, gy = o.qy - ky;
        const double g2 = gx * gx + gy * gy;
        if (k < 0 || g2 < kd) {                                // j + 1 only when strictly nearer
            k = kk;
            ex = fx;
            ey = fy;
            l2 = f2;
            kd = g2;
        }
    }
    if (k < 0) return false;
    const double len = sqrt(l2);
    o.j = best;
    o.nx = -ey / len;
    o.ny = ex / len;
    o.dx = o.qx - jx;
    o.dy = o.qy - jy;
    return true;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void keyframe_match_kernel(KeyframeArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ double s_ax[kMaxN], s_ay[kMaxN];
    __shared__ double s_part[kSums * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x, W = a.window;
    const long long row = (long long)b * N;
    const double qnan = __builtin_nan("");
    const float qnanf = __builtin_nanf("");
    int nd = 0;
    if (a.instance_mask) {
        nd = a.num_det[b];
        nd = nd < 0 ? 0 : (nd > N ? N : nd);
    }

    // slot c of thread t: beam t + THREADS * c.  The keyframe's vertex goes to LDS, the current point stays here
    double px[kSlots], py[kSlots];
    bool valid[kSlots];
    double votes[1] = {0.0};
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = tid + THREADS * c;
        px[c] = py[c] = 0.0;
        valid[c] = false;
        if (i < N) {
            const double cs = a.tab[N + 2 * i], sn = a.tab[N + 2 * i + 1];
            const float r0 = a.key_ranges[row + i], r1 = a.ranges_cur[row + i];
            const bool v0 = isfinite(r0) && (double)r0 < a.max_range;
            s_ax[i] = v0 ? (double)r0 * cs : qnan;
            s_ay[i] = v0 ? (double)r0 * sn : qnan;
            bool v1 = isfinite(r1) && (double)r1 < a.max_range;
            if (a.instance_mask) {
                const int id = a.instance_mask[row + i];
                if (id >= 1 && id <= nd && a.det_cls[row + id - 1] >= a.cls_thresh) v1 = false;
            }
            px[c] = (double)r1 * cs;
            py[c] = (double)r1 * sn;
            valid[c] = v1;
            if (v1) votes[0] += 1.0;
        }
    }
    const double phi0 = a.tab[0];
    const double dphi = N > 1 ? a.tab[1] - phi0 : 0.0;
    // the sensor's state, the same values in every thread
    const bool seeded = a.key_valid[b] != 0;
    const double x_old = a.pose[3 * b], y_old = a.pose[3 * b + 1], phi_old = a.pose[3 * b + 2];
    const double kx = a.key_pose[3 * b], ky = a.key_pose[3 * b + 1], kphi = a.key_pose[3 * b + 2];
    const int age = a.key_age[b], misses = a.key_misses[b];
    Rel m;
    m.th = m.ux = m.uy = 0.0;
    m.c = 1.0;
    m.s = 0.0;
    {
        const double t0 = a.key_rel[3 * b], t1 = a.key_rel[3 * b + 1], t2 = a.key_rel[3 * b + 2];
        if (isfinite(t0) && isfinite(t1) && isfinite(t2)) {
            m.th = t0;
            m.ux = t1;
            m.uy = t2;
        }
    }
    __syncthreads();                                           // the vertices are staged; the state is read
    group_sum<THREADS, 1>(votes, s_part);

    bool failed = true;
    int used = 0, matched = 0;
    double rms = qnan, obs = 0.0;
    if (seeded) {
        failed = false;
        for (int it = 0; it < a.iters; ++it) {
            sincos(m.th, &m.s, &m.c);
            double S[kSums];
#pragma unroll
            for (int k = 0; k < kSums; ++k) S[k] = 0.0;
#pragma unroll
            for (int c = 0; c < kSlots; ++c) {
                Match o;
                if (!valid[c] || !correspond(s_ax, s_ay, N, W, a.gate2, a.gap2, phi0, dphi, m, px[c], py[c], o))
                    continue;
                const double r = o.nx * o.dx + o.ny * o.dy;
                const double ar = fabs(r);
                const double w = (a.huber_delta > 0.0 && ar > a.huber_delta) ? a.huber_delta / ar : 1.0;
                const double j0 = o.nx * (-o.qy) + o.ny * o.qx, j1 = o.nx, j2 = o.ny;
                S[0] += w * (j0 * j0);
                S[1] += w * (j0 * j1);
                S[2] += w * (j0 * j2);
                S[3] += w * (j1 * j1);
                S[4] += w * (j1 * j2);
                S[5] += w * (j2 * j2);
                S[6] += w * (j0 * r);
                S[7] += w * (j1 * r);
                S[8] += w * (j2 * r);
                S[9] += w;
                S[10] += w * (r * r);
                S[11] += 1.0;
            }
            group_sum<THREADS, kSums>(S, s_part);
            used = it + 1;
            matched = (int)S[11];
            rms = sqrt(S[10] / S[9]);
            if (matched < 3) {
                failed = true;
                obs = 0.0;
                break;                                         // uniform: every thread holds the same bits
            }
            const double dmax = fmax(S[0], fmax(S[3], S[5]));
            const double floor_ = a.min_pivot * dmax;
            const double p0 = S[0];
            double pmin = p0, l00 = 0.0, l10 = 0.0, l20 = 0.0, l11 = 0.0, l21 = 0.0, l22 = 0.0;
            failed = !(p0 > floor_);
            if (!failed) {
                l00 = sqrt(p0);
                l10 = S[1] / l00;
                l20 = S[2] / l00;
                const double p1 = S[3] - l10 * l10;
                pmin = p1 < pmin ? p1 : pmin;
                failed = !(p1 > floor_);
                if (!failed) {
                    l11 = sqrt(p1);
                    l21 = (S[4] - l20 * l10) / l11;
                    const double p2 = (S[5] - l20 * l20) - l21 * l21;
                    pmin = p2 < pmin ? p2 : pmin;
                    failed = !(p2 > floor_);
                    if (!failed) l22 = sqrt(p2);
                }
            }
            obs = dmax > 0.0 ? pmin / dmax : 0.0;
            if (failed) break;
            const double y0 = -S[6] / l00;
            const double y1 = (-S[7] - l10 * y0) / l11;
            const double y2 = ((-S[8] - l20 * y0) - l21 * y1) / l22;
            const double x2 = y2 / l22;
            const double x1 = (y1 - l21 * x2) / l11;
            const double x0 = ((y0 - l10 * x1) - l20 * x2) / l00;
            double s0, c0;
            sincos(x0, &s0, &c0);
            const double nux = (c0 * m.ux - s0 * m.uy) + x1, nuy = (s0 * m.ux + c0 * m.uy) + x2;
            m.th = m.th + x0;
            m.ux = nux;
            m.uy = nuy;
            if (fabs(x0) < a.eps_theta && fmax(fabs(x1), fabs(x2)) < a.eps_u) break;
        }
    }

    // corr / flow_residual against the keyframe that was matched
    if (a.corr || a.flow_residual) {
        sincos(m.th, &m.s, &m.c);
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            const int i = tid + THREADS * c;
            if (i >= N) continue;
            Match o;
            const bool hit = !failed && valid[c] &&
                correspond(s_ax, s_ay, N, W, a.gate2, a.gap2, phi0, dphi, m, px[c], py[c], o);
            if (a.corr) a.corr[row + i] = hit ? o.j : -1;
            if (a.flow_residual) {
                a.flow_residual[2 * (row + i)] = hit ? m.c * o.dx + m.s * o.dy : qnan;
                a.flow_residual[2 * (row + i) + 1] = hit ? (-m.s) * o.dx + m.c * o.dy : qnan;
            }
        }
    }

    // the policy: the same decision in every thread
    double x_new = x_old, y_new = y_old, phi_new = phi_old;
    bool replace;
    int new_age, new_misses;
    if (!seeded) {
        replace = true;
        new_age = 0;
        new_misses = 0;
    } else if (!failed) {
        double sk, ck;
        sincos(kphi, &sk, &ck);
        phi_new = kphi + m.th;
        x_new = kx + (ck * m.ux - sk * m.uy);
        y_new = ky + (sk * m.ux + ck * m.uy);
        replace = fabs(m.th) > a.key_rot || m.ux * m.ux + m.uy * m.uy > a.key_dist2 ||
            (double)matched < a.min_share * votes[0];
        new_age = replace ? 0 : age + 1;
        new_misses = 0;
    } else {
        replace = misses + 1 > a.max_misses;
        new_age = replace ? 0 : age + 1;
        new_misses = replace ? 0 : misses + 1;
    }
    if (replace) {
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            const int i = tid + THREADS * c;
            if (i < N) a.key_ranges[row + i] = valid[c] ? a.ranges_cur[row + i] : qnanf;
        }
    }
    if (tid == 0) {
        const bool good = seeded && !failed;
        a.motion[3 * b] = good ? m.th : qnan;
        a.motion[3 * b + 1] = good ? m.ux : qnan;
        a.motion[3 * b + 2] = good ? m.uy : qnan;
        a.count[b] = matched;
        a.rms[b] = good ? rms : qnan;
        a.ok[b] = good ? 1 : 0;
        a.iters_used[b] = used;
        a.obs[b] = obs;
        a.key_replaced[b] = replace ? 1 : 0;
        a.pose[3 * b] = x_new;
        a.pose[3 * b + 1] = y_new;
        a.pose[3 * b + 2] = phi_new;
        if (replace) {
            a.key_pose[3 * b] = x_new;
            a.key_pose[3 * b + 1] = y_new;
            a.key_pose[3 * b + 2] = phi_new;
            a.key_rel[3 * b] = a.key_rel[3 * b + 1] = a.key_rel[3 * b + 2] = 0.0;
        } else if (good) {
            a.key_rel[3 * b] = m.th;
            a.key_rel[3 * b + 1] = m.ux;
            a.key_rel[3 * b + 2] = m.uy;
        }
        a.key_valid[b] = 1;
        a.key_age[b] = new_age;
        a.key_misses[b] = new_misses;
        if (a.rot) {
            double s1, c1;
            sincos(phi_new, &s1, &c1);
            a.rot[4 * b] = (float)c1;
            a.rot[4 * b + 1] = (float)(-s1);
            a.rot[4 * b + 2] = (float)s1;
            a.rot[4 * b + 3] = (float)c1;
        }
        if (a.trans) {
            a.trans[2 * b] = x_new;
            a.trans[2 * b + 1] = y_new;
        }
        if (a.flow_trans) {
            a.flow_trans[2 * b] = good ? x_new - x_old : 0.0;
            a.flow_trans[2 * b + 1] = good ? y_new - y_old : 0.0;
        }
    }
}

}  // namespace

extern "C" int pof_keyframe_match(const float *ranges_cur, const double *tab, const int32_t *instance_mask,
                                  const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range,
                                  int window, double gate, double max_gap, double huber_delta, int iters,
                                  double eps_theta, double eps_u, double min_pivot, double key_dist, double key_rot,
                                  double min_share, int max_misses, int B, int N, float *key_ranges, double *key_pose,
                                  double *key_rel, uint8_t *key_valid, int32_t *key_age, int32_t *key_misses,
                                  double *pose, double *motion, int32_t *count, double *rms, uint8_t *ok,
                                  int32_t *iters_used, double *obs, uint8_t *key_replaced, int32_t *corr,
                                  double *flow_residual, float *rot, double *trans, double *flow_trans,
                                  pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges_cur || !tab || !key_ranges || !key_pose || !key_rel || !key_valid || !key_age || !key_misses || !pose)
        return POF_E_BADARG;
    if (!motion || !count || !rms || !ok || !iters_used || !obs || !key_replaced) return POF_E_BADARG;
    if (window < 1 || window > kMaxWindow || iters < 1 || iters > kMaxIters) return POF_E_BADARG;
    if (!(gate >= 0.0) || !(max_gap >= 0.0) || !(huber_delta >= 0.0)) return POF_E_BADARG;
    if (!(key_dist >= 0.0) || !(key_rot >= 0.0) || !(min_share >= 0.0) || max_misses < 0) return POF_E_BADARG;
    if (instance_mask && (!num_det || !det_cls)) return POF_E_BADARG;
    if (B < 0 || N < 1) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_scan_match and the NMS
    if (B == 0) return POF_OK;
    KeyframeArgs a;
    a.ranges_cur = ranges_cur; a.tab = tab; a.instance_mask = instance_mask; a.num_det = num_det; a.det_cls = det_cls;
    a.cls_thresh = cls_thresh; a.max_range = max_range; a.gate2 = gate * gate; a.gap2 = max_gap * max_gap;
    a.huber_delta = huber_delta; a.eps_theta = eps_theta; a.eps_u = eps_u; a.min_pivot = min_pivot;
    a.key_rot = key_rot; a.key_dist2 = key_dist * key_dist; a.min_share = min_share; a.window = window;
    a.iters = iters; a.max_misses = max_misses; a.N = N;
    a.key_ranges = key_ranges; a.key_pose = key_pose; a.key_rel = key_rel; a.key_valid = key_valid;
    a.key_age = key_age; a.key_misses = key_misses; a.pose = pose;
    a.motion = motion; a.count = count; a.rms = rms; a.ok = ok; a.iters_used = iters_used; a.obs = obs;
    a.key_replaced = key_replaced; a.corr = corr; a.flow_residual = flow_residual; a.rot = rot; a.trans = trans;
    a.flow_trans = flow_trans;
    if (N <= kWaveMaxN)
        keyframe_match_kernel<64><<<B, 64, 0, pof_stream(stream)>>>(a);
    else
        keyframe_match_kernel<kGroupThreads><<<B, kGroupThreads, 0, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
