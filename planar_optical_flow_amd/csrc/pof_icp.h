// The point-to-line ICP core of pof_scan_match (N8, scan_match.hip) and of pof_keyframe_match and
// pof_keyframe_map_match (N9 and N10, one kernel in keyframe_match.hip): one copy of every formula.  The two kernels
// differ in where the search window of a point is centred (a functor, below), in what feeds the start value and in
// what they do with the result; everything here they share operation for operation.
// Restated in float64 NumPy by tests/test_scan_match.py (_correspond, _iterate).
//
// Reference vertices a_j, current points p_i, gate2 = gate * gate, gap2 = max_gap * max_gap.
//
// Correspondence of p at (theta, u), with (c, s) = (cos theta, sin theta):
//   q = ((c p_x - s p_y) + u_x, (s p_x + c p_y) + u_y)
//   mid = the window centre of point i: a functor with set(theta), called once per pass, and (i, q_x, q_y) -> mid
//   j = the valid vertex of smallest d2 = (q_x - a_jx)^2 + (q_y - a_jy)^2 over
//       [mid - W, mid + W] n [0, N), scanned upwards with a strict <: ties go to the lower j.
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
// The reference vertices are staged once in LDS (two doubles per beam, NaN = not valid; 64 KB at N = 4096).  Thread t
// holds the points t, t + THREADS, ... in kSlots register slots and adds them in slot order; the sums meet in
// group_sum (pof_common.h): the per-sensor workgroup of pof_sensor.h, its slot layout, launch forms and fixed order.
// Every lane ends with the same bits, solves redundantly, and the iteration loop and its exit are uniform.
#pragma once
#include <cmath>

#include "pof_sensor.h"

namespace pof_icp {

using pof_sensor::kGroupMaxN;
using pof_sensor::kGroupThreads;
using pof_sensor::kSlots;
using pof_sensor::kWaveMaxN;
constexpr int kMaxIters = 32;
constexpr int kMaxWindow = 64;
constexpr int kSums = 12;

// what both matchers read of the current scan: the ranges, the angle table and the NMS gate
struct Input {
    const float *ranges_cur;
    const double *tab;
    pof_sensor::NmsGate gate;
    double max_range;
};

// Input and Settings are passed by value, and window / gate2 / gap2 to `correspond` as scalars: through references the
// compiler loses its no-clobber annotation of the kernel-argument loads.
struct Settings {
    double gate2, gap2, huber_delta, eps_theta, eps_u, min_pivot;
    int window, iters;
};

struct Pose {
    double th, ux, uy, c, s;
};

struct Match {
    int j;
    double qx, qy, dx, dy, nx, ny;
};

struct Result {
    bool failed;
    int used, matched;
    double rms, obs;
};

// The launchers' checks of the settings, the gate and the sizes -> POF_OK or POF_E_BADARG.
inline int check_settings(int window, double gate, double max_gap, double huber_delta, int iters,
                          const int32_t *instance_mask, const int32_t *num_det, const double *det_cls, int B, int N)
{
    if (window < 1 || window > kMaxWindow || iters < 1 || iters > kMaxIters) return POF_E_BADARG;
    if (!(gate >= 0.0) || !(max_gap >= 0.0) || !(huber_delta >= 0.0)) return POF_E_BADARG;
    if (instance_mask && (!num_det || !det_cls)) return POF_E_BADARG;
    if (B < 0 || N < 1) return POF_E_BADARG;
    return POF_OK;
}

// Staging of workgroup b.  Slot c of thread t: beam t + THREADS * c.  The reference scan's vertex goes to LDS, the
// current point stays in the slots; a current point is not valid when its range is not finite or >= max_range or it
// belongs to a detection of score >= cls_thresh.  -> the number of valid points of this thread.
template <int THREADS>
__device__ __forceinline__ double stage(const Input in, const float *ranges_ref, int b, int N, double *ax, double *ay,
                                        double (&px)[kSlots], double (&py)[kSlots], bool (&valid)[kSlots])
{
    const int tid = threadIdx.x;
    const long long row = (long long)b * N;
    const double qnan = __builtin_nan("");
    const int nd = in.gate.num(b, N);
    double votes = 0.0;
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = tid + THREADS * c;
        px[c] = py[c] = 0.0;
        valid[c] = false;
        if (i < N) {
            const double cs = in.tab[N + 2 * i], sn = in.tab[N + 2 * i + 1];
            const float r0 = ranges_ref[row + i], r1 = in.ranges_cur[row + i];
            const bool v0 = isfinite(r0) && (double)r0 < in.max_range;
            ax[i] = v0 ? (double)r0 * cs : qnan;
            ay[i] = v0 ? (double)r0 * sn : qnan;
            bool v1 = isfinite(r1) && (double)r1 < in.max_range;
            if (in.gate.is_person(row, i, nd)) v1 = false;
            px[c] = (double)r1 * cs;
            py[c] = (double)r1 * sn;
            valid[c] = v1;
            if (v1) votes += 1.0;
        }
    }
    return votes;
}

// the correspondence of point i = (px, py); ax / ay: the staged vertices, every index read lies in [0, N)
template <class Centre>
__device__ __forceinline__ bool correspond(const double *ax, const double *ay, int N, int W, double gate2, double gap2,
                                           const Centre &centre, const Pose &m, int i, double px, double py, Match &o)
{
    o.qx = (m.c * px - m.s * py) + m.ux;
    o.qy = (m.s * px + m.c * py) + m.uy;
    const int mid = centre(i, o.qx, o.qy);                     // in [-N, 2N], N <= 4096: no overflow
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

// The 3 x 3 solve of the header comment, shared with pof_grid_refine (N19, grid_refine.hip): A x = -g with A = (A00 A01
// A02; . A11 A12; . . A22) by Cholesky, every pivot tested against min_pivot * dmax as it is formed; obs as above.  x
// is not formed when a pivot fails.
struct Solve3 {
    bool failed;
    double obs, x0, x1, x2;
};

__device__ __forceinline__ Solve3 cholesky3(double A00, double A01, double A02, double A11, double A12, double A22,
                                            double g0, double g1, double g2, double min_pivot)
{
    Solve3 o = {false, 0.0, 0.0, 0.0, 0.0};
    const double dmax = fmax(A00, fmax(A11, A22));
    const double floor_ = min_pivot * dmax;
    const double p0 = A00;
    double pmin = p0, l00 = 0.0, l10 = 0.0, l20 = 0.0, l11 = 0.0, l21 = 0.0, l22 = 0.0;
    o.failed = !(p0 > floor_);
    if (!o.failed) {
        l00 = sqrt(p0);
        l10 = A01 / l00;
        l20 = A02 / l00;
        const double p1 = A11 - l10 * l10;
        pmin = p1 < pmin ? p1 : pmin;
        o.failed = !(p1 > floor_);
        if (!o.failed) {
            l11 = sqrt(p1);
            l21 = (A12 - l20 * l10) / l11;
            const double p2 = (A22 - l20 * l20) - l21 * l21;
            pmin = p2 < pmin ? p2 : pmin;
            o.failed = !(p2 > floor_);
            if (!o.failed) l22 = sqrt(p2);
        }
    }
    o.obs = dmax > 0.0 ? pmin / dmax : 0.0;
    if (o.failed) return o;
    const double y0 = -g0 / l00;
    const double y1 = (-g1 - l10 * y0) / l11;
    const double y2 = ((-g2 - l20 * y0) - l21 * y1) / l22;
    o.x2 = y2 / l22;
    o.x1 = (y1 - l21 * o.x2) / l11;
    o.x0 = ((y0 - l10 * o.x1) - l20 * o.x2) / l00;
    return o;
}

// The iterations from the start value in m, which ends as the final (theta, u).  `part`: the LDS of group_sum<kSums>.
template <int THREADS, class Centre>
__device__ __forceinline__ Result iterate(const double *ax, const double *ay, double *part, int N, const Settings st,
                                          Centre &centre, const double (&px)[kSlots], const double (&py)[kSlots],
                                          const bool (&valid)[kSlots], Pose &m)
{
    const int tid = threadIdx.x;
    Result res = {false, 0, 0, __builtin_nan(""), 0.0};
    for (int it = 0; it < st.iters; ++it) {
        sincos(m.th, &m.s, &m.c);
        centre.set(m.th);
        double S[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) S[k] = 0.0;
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            Match o;
            if (!valid[c] || !correspond(ax, ay, N, st.window, st.gate2, st.gap2, centre, m, tid + THREADS * c, px[c],
                                         py[c], o))
                continue;
            const double r = o.nx * o.dx + o.ny * o.dy;
            const double ar = fabs(r);
            const double w = (st.huber_delta > 0.0 && ar > st.huber_delta) ? st.huber_delta / ar : 1.0;
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
        group_sum<THREADS, kSums>(S, part);
        res.used = it + 1;
        res.matched = (int)S[11];
        res.rms = sqrt(S[10] / S[9]);
        if (res.matched < 3) {
            res.failed = true;
            res.obs = 0.0;
            break;                                             // uniform: every thread holds the same bits
        }
        const Solve3 sol = cholesky3(S[0], S[1], S[2], S[3], S[4], S[5], S[6], S[7], S[8], st.min_pivot);
        res.failed = sol.failed;
        res.obs = sol.obs;
        if (res.failed) break;
        const double x0 = sol.x0, x1 = sol.x1, x2 = sol.x2;
        double s0, c0;
        sincos(x0, &s0, &c0);
        const double nux = (c0 * m.ux - s0 * m.uy) + x1, nuy = (s0 * m.ux + c0 * m.uy) + x2;
        m.th = m.th + x0;
        m.ux = nux;
        m.uy = nuy;
        if (fabs(x0) < st.eps_theta && fmax(fabs(x1), fabs(x2)) < st.eps_u) break;
    }
    return res;
}

// corr / flow_residual of row b (either may be NULL) at the final (theta, u) in m; all -1 / NaN when `failed`.
template <int THREADS, class Centre>
__device__ __forceinline__ void write_corr(const double *ax, const double *ay, int b, int N, const Settings st,
                                           Centre &centre, const double (&px)[kSlots], const double (&py)[kSlots],
                                           const bool (&valid)[kSlots], Pose &m, bool failed, int32_t *corr,
                                           double *flow_residual)
{
    if (!corr && !flow_residual) return;
    const int tid = threadIdx.x;
    const long long row = (long long)b * N;
    const double qnan = __builtin_nan("");
    sincos(m.th, &m.s, &m.c);
    centre.set(m.th);
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = tid + THREADS * c;
        if (i >= N) continue;
        Match o;
        const bool hit = !failed && valid[c] &&
            correspond(ax, ay, N, st.window, st.gate2, st.gap2, centre, m, i, px[c], py[c], o);
        if (corr) corr[row + i] = hit ? o.j : -1;
        if (flow_residual) {
            flow_residual[2 * (row + i)] = hit ? m.c * o.dx + m.s * o.dy : qnan;
            flow_residual[2 * (row + i) + 1] = hit ? (-m.s) * o.dx + m.c * o.dy : qnan;
        }
    }
}

}  // namespace pof_icp
