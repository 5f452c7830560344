// N8: the sensor's own motion between two consecutive scans without a flow field -- a point-to-line ICP of the
// current scan against the previous one, one launch per batch, one scan pair per workgroup.  On a static scene the
// result inverts get_displacement_from_odometry (src/utils/utils.py:639-662); it has the (theta, u) convention of
// pof_ego_motion's rigid model (a point now at p was at R(theta) p + u), so pof_pose_advance takes it unchanged.
// The reference has no scan matcher: the specification is this comment, restated in float64 NumPy by
// tests/test_scan_match.py (match_oracle).
//
// Points.  a_j = r_prev[j] * (cos, sin)[j], p_i = r_cur[i] * (cos, sin)[i] in float64 from the angle table, as
// rphi_to_xy.  A range is valid when it is finite and < max_range.  A current point is also left out when it belongs
// to a detection of score >= cls_thresh (instance_mask, num_det, det_cls as in pof_ego_motion; people do not vote).
// dphi = tab[1] - tab[0] (0 for N = 1).  Start: (theta, u) = init row, zeros when init is NULL or the row has a
// component that is not finite.  gate2 = gate * gate, gap2 = max_gap * max_gap.
//
// Correspondence of p at (theta, u), with (c, s) = (cos theta, sin theta):
//   shift = (int)clamp(rint(theta / dphi), -N, N)   (0 when dphi == 0; a NaN quotient gives -N)
//   q = ((c p_x - s p_y) + u_x, (s p_x + c p_y) + u_y)
//   j = the valid vertex of smallest d2 = (q_x - a_jx)^2 + (q_y - a_jy)^2 over
//       [i + shift - W, i + shift + W] n [0, N), scanned upwards with a strict <: ties go to the lower j.
//       Unmatched without one or when not d2 <= gate2.
//   k in {j - 1, j + 1}: in [0, N), valid, e = a_k - a_j with 0 < |e|^2 <= gap2.  Of two that qualify the one with
//       the smaller |q - a_k|^2, j - 1 on a tie.  Unmatched without one.
//   len = sqrt(|e|^2), n = (-e_y / len, e_x / len), d = q - a_j, r = n_x d_x + n_y d_y
// One iteration:
//   w = |r| > huber_delta ? huber_delta / |r| : 1 (1 when huber_delta == 0),  J = (n_x (-q_y) + n_y q_x, n_x, n_y)
//   twelve sums over the matched points: w (J_a J_b) for ab = 00 01 02 11 12 22 -> A, w (J_a r) -> g, w, w (r r), 1.
//   Fails with fewer than 3 matched points (obs = 0).  dmax = max(A00, A11, A22).  Cholesky, every pivot tested as it
//   is formed; the pair fails at the first pivot that is not > min_pivot * dmax:
//     p0 = A00, l00 = sqrt(p0), l10 = A01 / l00, l20 = A02 / l00
//     p1 = A11 - l10 l10, l11 = sqrt(p1), l21 = (A12 - l20 l10) / l11
//     p2 = (A22 - l20 l20) - l21 l21, l22 = sqrt(p2)
//     obs = min(pivots formed) / dmax (0 when dmax is not > 0)
//     y0 = -g0 / l00, y1 = (-g1 - l10 y0) / l11, y2 = ((-g2 - l20 y0) - l21 y1) / l22
//     x2 = y2 / l22, x1 = (y1 - l21 x2) / l11, x0 = ((y0 - l10 x1) - l20 x2) / l00
//   (c0, s0) = (cos x0, sin x0):  theta += x0,  u <- ((c0 u_x - s0 u_y) + x1, (s0 u_x + c0 u_y) + x2)
//   count, rms = sqrt(sum w r r / sum w), obs and iters_used are those of the last iteration run.
//   Stop after `iters` iterations or when |x0| < eps_theta and max(|x1|, |x2|) < eps_u.
//   A failed pair: ok = 0, motion and rms NaN, corr -1, flow_residual NaN.
// Afterwards one more correspondence pass at the final (theta, u): corr[i] = j, flow_residual[i] =
// (c d_x + s d_y, -s d_x + c d_y), the nearest-vertex displacement turned back into the current scanner frame;
// -1 / NaN where unmatched.
//
// The previous scan's vertices are staged once in LDS (two doubles per beam, NaN = not valid; 64 KB at N = 4096).
// Thread t holds the points t, t + THREADS, ... in kSlots register slots and adds them in slot order; the lanes of a
// wave meet in a float64 __shfl_xor butterfly, the 8 wave totals of the 512-thread form go through LDS and every
// thread adds them in wave order: a FIXED ORDER, no atomics, and with -ffp-contract=off no FMA.  Every lane ends with
// the same bits, solves redundantly, and the iteration loop and its exit are uniform.
//   N <= 512:  one wave per pair;   N <= 4096: 512 threads per pair.
// init may be the motion buffer: a workgroup reads its row before it writes it.
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

struct ScanMatchArgs {
    const float *ranges_prev, *ranges_cur;
    const double *tab, *init;
    const int32_t *instance_mask, *num_det;
    const double *det_cls;
    double cls_thresh, max_range, gate2, gap2, huber_delta, eps_theta, eps_u, min_pivot;
    int window, iters, N;
    double *motion;
    int32_t *count;
    double *rms;
    uint8_t *ok;
    int32_t *iters_used;
    double *obs;
    int32_t *corr;
    double *flow_residual;
};

// Sum of K values over the workgroup, the same bits in every thread (as in ego_motion.hip).  `part` is [K][8]
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

struct Pose {
    double th, ux, uy, c, s;
    int shift;
};

struct Match {
    int j;
    double qx, qy, dx, dy, nx, ny;
};

__device__ __forceinline__ int beam_shift(double th, double dphi, int N)
{
    if (dphi == 0.0) return 0;
    double t = rint(th / dphi);
    if (!(t >= (double)-N)) t = (double)-N;
    if (!(t <= (double)N)) t = (double)N;
    return (int)t;
}

// the correspondence of point i = (px, py); ax / ay: the staged vertices, every index read lies in [0, N)
__device__ __forceinline__ bool correspond(const double *ax, const double *ay, int N, int W, double gate2, double gap2,
                                           const Pose &m, int i, double px, double py, Match &o)
{
    o.qx = (m.c * px - m.s * py) + m.ux;
    o.qy = (m.s * px + m.c * py) + m.uy;
    const int mid = i + m.shift;                               // |shift| <= N <= 4096: no overflow
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
__global__ __launch_bounds__(THREADS) void scan_match_kernel(ScanMatchArgs a)
{
    constexpr int kMaxN = THREADS * kSlots;
    __shared__ double s_ax[kMaxN], s_ay[kMaxN];
    __shared__ double s_part[kSums * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x, W = a.window;
    const long long row = (long long)b * N;
    const double qnan = __builtin_nan("");
    int nd = 0;
    if (a.instance_mask) {
        nd = a.num_det[b];
        nd = nd < 0 ? 0 : (nd > N ? N : nd);
    }

    // slot c of thread t: beam t + THREADS * c.  The previous scan's vertex goes to LDS, the current point stays here
    double px[kSlots], py[kSlots];
    bool valid[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = tid + THREADS * c;
        px[c] = py[c] = 0.0;
        valid[c] = false;
        if (i < N) {
            const double cs = a.tab[N + 2 * i], sn = a.tab[N + 2 * i + 1];
            const float r0 = a.ranges_prev[row + i], r1 = a.ranges_cur[row + i];
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
        }
    }
    const double dphi = N > 1 ? a.tab[1] - a.tab[0] : 0.0;
    Pose m;
    m.th = m.ux = m.uy = 0.0;
    if (a.init) {
        const double t0 = a.init[3 * b], t1 = a.init[3 * b + 1], t2 = a.init[3 * b + 2];
        if (isfinite(t0) && isfinite(t1) && isfinite(t2)) {
            m.th = t0;
            m.ux = t1;
            m.uy = t2;
        }
    }
    __syncthreads();                                           // the vertices are staged; init is read

    bool failed = false;
    int used = 0, matched = 0;
    double rms = qnan, obs = 0.0;
    for (int it = 0; it < a.iters; ++it) {
        sincos(m.th, &m.s, &m.c);
        m.shift = beam_shift(m.th, dphi, N);
        double S[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) S[k] = 0.0;
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            Match o;
            if (!valid[c] || !correspond(s_ax, s_ay, N, W, a.gate2, a.gap2, m, tid + THREADS * c, px[c], py[c], o))
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
            break;                                             // uniform: every thread holds the same bits
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

    if (a.corr || a.flow_residual) {
        sincos(m.th, &m.s, &m.c);
        m.shift = beam_shift(m.th, dphi, N);
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            const int i = tid + THREADS * c;
            if (i >= N) continue;
            Match o;
            const bool hit = !failed && valid[c] &&
                correspond(s_ax, s_ay, N, W, a.gate2, a.gap2, m, i, px[c], py[c], o);
            if (a.corr) a.corr[row + i] = hit ? o.j : -1;
            if (a.flow_residual) {
                a.flow_residual[2 * (row + i)] = hit ? m.c * o.dx + m.s * o.dy : qnan;
                a.flow_residual[2 * (row + i) + 1] = hit ? (-m.s) * o.dx + m.c * o.dy : qnan;
            }
        }
    }
    if (tid == 0) {
        a.motion[3 * b] = failed ? qnan : m.th;
        a.motion[3 * b + 1] = failed ? qnan : m.ux;
        a.motion[3 * b + 2] = failed ? qnan : m.uy;
        a.count[b] = matched;
        a.rms[b] = failed ? qnan : rms;
        a.ok[b] = failed ? 0 : 1;
        a.iters_used[b] = used;
        a.obs[b] = obs;
    }
}

}  // namespace

extern "C" int pof_scan_match(const float *ranges_prev, const float *ranges_cur, const double *tab, const double *init,
                              const int32_t *instance_mask, const int32_t *num_det, const double *det_cls,
                              double cls_thresh, double max_range, int window, double gate, double max_gap,
                              double huber_delta, int iters, double eps_theta, double eps_u, double min_pivot, int B,
                              int N, double *motion, int32_t *count, double *rms, uint8_t *ok, int32_t *iters_used,
                              double *obs, int32_t *corr, double *flow_residual, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!ranges_prev || !ranges_cur || !tab || !motion || !count || !rms || !ok || !iters_used || !obs)
        return POF_E_BADARG;
    if (window < 1 || window > kMaxWindow || iters < 1 || iters > kMaxIters) return POF_E_BADARG;
    if (!(gate >= 0.0) || !(max_gap >= 0.0) || !(huber_delta >= 0.0)) return POF_E_BADARG;
    if (instance_mask && (!num_det || !det_cls)) return POF_E_BADARG;
    if (B < 0 || N < 1) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_ego_motion and the NMS
    if (B == 0) return POF_OK;
    ScanMatchArgs a;
    a.ranges_prev = ranges_prev; a.ranges_cur = ranges_cur; a.tab = tab; a.init = init;
    a.instance_mask = instance_mask; a.num_det = num_det; a.det_cls = det_cls; a.cls_thresh = cls_thresh;
    a.max_range = max_range; a.gate2 = gate * gate; a.gap2 = max_gap * max_gap; a.huber_delta = huber_delta;
    a.eps_theta = eps_theta; a.eps_u = eps_u; a.min_pivot = min_pivot; a.window = window; a.iters = iters; a.N = N;
    a.motion = motion; a.count = count; a.rms = rms; a.ok = ok; a.iters_used = iters_used; a.obs = obs; a.corr = corr;
    a.flow_residual = flow_residual;
    if (N <= kWaveMaxN)
        scan_match_kernel<64><<<B, 64, 0, pof_stream(stream)>>>(a);
    else
        scan_match_kernel<kGroupThreads><<<B, kGroupThreads, 0, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
