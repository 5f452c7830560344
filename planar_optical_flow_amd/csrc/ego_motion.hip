// N6: the sensor's own motion from a flow field, one launch per batch: the weighted least-squares inverse of
// get_displacement_from_odometry (src/utils/utils.py:639-662) and get_velocity_from_odometry (:609-636).
//
// Per point i of scan b:  p = xy (or r * (cos, sin) as rphi_to_xy),  f = the flow, rotated out of the canonical frame
// by pof_rotate_flow_point in its own type when canonical != 0,  g = sign * f,  q = p + g.  Base weight w0 = weight
// (or 1); 0 when the weight is not finite or <= 0, the range not finite or >= max_range, a flow or point component
// not finite, or the point belongs to a detection with det_cls >= cls_thresh (pof_person_flow's det_valid).
// Solve with weights w (only terms with w > 0 enter a sum, so a gated NaN stays out):
//   W = sum w, pm = sum w p / W, qm = sum w q / W;  p' = p - pm, q' = q - qm
//   S_pp = sum w |p'|^2,  S_dot = sum w p'.q',  S_x = sum w (p'_x q'_y - p'_y q'_x)
//   model 0 (rigid):  theta = atan2(S_x, S_dot),  u = qm - R(theta) pm,            e = R(theta) p + u - q
//   model 1 (linear): gm = sum w g / W, g' = g - gm,  omega = sum w (p'_x g'_y - p'_y g'_x) / S_pp,
//                     t = gm - omega (-pm_y, pm_x),                                 e = t + omega (-y, x) - g
// A solve fails with fewer than two points of w > 0 or S_pp not > 0.  Huber: w = w0 * (|e| > delta ? delta / |e| : 1),
// `iters` times, i.e. iters + 1 solves.
//
// The per-sensor workgroup of pof_sensor.h: thread t holds the points t, t + THREADS, ... in kSlots register slots
// (coalesced loads) and adds them in slot order; the 64 lanes of a wave meet in a float64 __shfl_xor butterfly.  A
// butterfly stage adds the same two numbers in both lanes and IEEE addition is commutative, so all 64 lanes end with
// the same bits and every lane solves redundantly -- no broadcast.
//   N <= 512:  one wave per scan, no LDS;
//   N <= 4096: 512 threads per scan; the 8 wave totals go through LDS and every thread adds them in wave order.
// The same bits in every run, at every batch position and in a graph replay.  Built with -ffp-contract=off: no FMA.
// Latency bound like the NMS and the per-person launch it sits between.
//
// pof_pose_advance: one thread per scan composes the fitted motion (displacement convention) onto a pose and writes
// the three terms pof_person_flow reads.
#include <cmath>

#include "pof_sensor.h"

namespace {

using namespace pof_sensor;

constexpr int kMaxIters = 16;

struct EgoMotionArgs {
    const float *ranges;
    const double *xy, *tab;
    const void *flow;
    const float *weight;
    NmsGate gate;
    double max_range, huber_delta;
    int flow_f64, canonical, sign, model, iters, N;
    double *motion;
    int32_t *count;
    double *rms;
    uint8_t *ok;
    double *flow_residual;
    float *weight_out;
};

struct Solution {
    double a, b0, b1;      // (theta, u) or (omega, t)
    double c, s;           // cos / sin of theta (rigid)
    double W;
};

// h is q for the rigid model and g for the linear one
__device__ __forceinline__ void residual(int model, const Solution &m, double px, double py, double hx, double hy,
                                         double &ex, double &ey)
{
    if (model == 0) {
        ex = (m.c * px - m.s * py) + m.b0 - hx;
        ey = (m.s * px + m.c * py) + m.b1 - hy;
    } else {
        ex = (m.b0 + m.a * (-py)) - hx;
        ey = (m.b1 + m.a * px) - hy;
    }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void ego_motion_kernel(EgoMotionArgs a)
{
    __shared__ double s_part[6 * (THREADS > 64 ? THREADS / 64 : 1)];
    const int N = a.N, b = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)b * N;
    const double sgn = (double)a.sign;
    const int nd = a.gate.num(b, N);

    // slot c of thread t: point t + THREADS * c.  p, h (= q = p + g for the rigid model, g for the linear one), the
    // base weight and the weight of the solve at hand
    double px[kSlots], py[kSlots], hx[kSlots], hy[kSlots], w0[kSlots], w[kSlots];
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = tid + THREADS * c;
        px[c] = py[c] = hx[c] = hy[c] = w0[c] = 0.0;
        if (i < N) {
            const long long p = row + i;
            double cs = 0.0, sn = 0.0;
            if (a.tab) {
                cs = a.tab[N + 2 * i];
                sn = a.tab[N + 2 * i + 1];
            }
            double wt = a.weight ? (double)a.weight[p] : 1.0;
            if (!(wt > 0.0) || !isfinite(wt)) wt = 0.0;
            if (a.ranges) {
                const float r = a.ranges[p];
                if (!isfinite(r) || !((double)r < a.max_range)) wt = 0.0;
                if (!a.xy) {
                    px[c] = (double)r * cs;
                    py[c] = (double)r * sn;
                }
            }
            if (a.xy) {
                px[c] = a.xy[2 * p];
                py[c] = a.xy[2 * p + 1];
            }
            double fx, fy;
            if (a.flow_f64) {
                double f0 = ((const double *)a.flow)[2 * p], f1 = ((const double *)a.flow)[2 * p + 1];
                if (a.canonical) pof_rotate_flow_point<double>(cs, sn, f0, f1, 0, f0, f1);
                fx = f0;
                fy = f1;
            } else {
                float f0 = ((const float *)a.flow)[2 * p], f1 = ((const float *)a.flow)[2 * p + 1];
                if (a.canonical) pof_rotate_flow_point<float>(cs, sn, f0, f1, 0, f0, f1);
                fx = (double)f0;
                fy = (double)f1;
            }
            if (!isfinite(fx) || !isfinite(fy) || !isfinite(px[c]) || !isfinite(py[c])) wt = 0.0;
            if (a.gate.is_person(row, i, nd)) wt = 0.0;
            hx[c] = sgn * fx;
            hy[c] = sgn * fy;
            if (a.model == 0) {
                hx[c] = px[c] + hx[c];
                hy[c] = py[c] + hy[c];
            }
            w0[c] = wt;
        }
        w[c] = w0[c];
    }

    const double qnan = __builtin_nan("");
    const int n_it = a.huber_delta > 0.0 ? a.iters : 0;
    Solution m;
    bool failed = false;
    for (int it = 0;; ++it) {
        // first pass: total weight, the weighted means, the number of points that count
        double s1[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            if (w[c] > 0.0) {
                s1[0] += w[c];
                s1[1] += w[c] * px[c];
                s1[2] += w[c] * py[c];
                s1[3] += w[c] * hx[c];
                s1[4] += w[c] * hy[c];
                s1[5] += 1.0;
            }
        }
        group_sum<THREADS, 6>(s1, s_part);
        const double W = s1[0];
        const double pmx = s1[1] / W, pmy = s1[2] / W, hmx = s1[3] / W, hmy = s1[4] / W;
        // second pass over the registers: the centred moments
        double s2[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            if (w[c] > 0.0) {
                const double dx = px[c] - pmx, dy = py[c] - pmy, ex = hx[c] - hmx, ey = hy[c] - hmy;
                s2[0] += w[c] * (dx * dx + dy * dy);
                s2[1] += w[c] * (dx * ex + dy * ey);
                s2[2] += w[c] * (dx * ey - dy * ex);
            }
        }
        group_sum<THREADS, 3>(s2, s_part);
        m.W = W;
        if (s1[5] < 2.0 || !(s2[0] > 0.0)) {
            failed = true;
            m.a = m.b0 = m.b1 = m.c = m.s = qnan;
        } else if (a.model == 0) {
            m.a = atan2(s2[2], s2[1]);
            sincos(m.a, &m.s, &m.c);
            m.b0 = hmx - (m.c * pmx - m.s * pmy);
            m.b1 = hmy - (m.s * pmx + m.c * pmy);
        } else {
            m.a = s2[2] / s2[0];
            m.c = m.s = 0.0;
            m.b0 = hmx - m.a * (-pmy);
            m.b1 = hmy - m.a * pmx;
        }
        if (failed || it >= n_it) break;                       // uniform: every thread holds the same bits
#pragma unroll
        for (int c = 0; c < kSlots; ++c) {
            double ex, ey;
            residual(a.model, m, px[c], py[c], hx[c], hy[c], ex, ey);
            const double rho = hypot(ex, ey);
            w[c] = w0[c] * (rho > a.huber_delta ? a.huber_delta / rho : 1.0);
        }
    }

    // residuals of the last solve: rms, the ego-compensated flow and the weights
    double sr[2] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int i = tid + THREADS * c;
        double ex, ey;
        residual(a.model, m, px[c], py[c], hx[c], hy[c], ex, ey);
        if (w[c] > 0.0) {
            const double rho = hypot(ex, ey);
            sr[0] += w[c] * (rho * rho);
        }
        if (w0[c] > 0.0) sr[1] += 1.0;
        if (i < N) {
            const long long p = row + i;
            if (a.flow_residual) {
                a.flow_residual[2 * p] = -sgn * ex;
                a.flow_residual[2 * p + 1] = -sgn * ey;
            }
            if (a.weight_out) a.weight_out[p] = (float)w[c];
        }
    }
    group_sum<THREADS, 2>(sr, s_part);
    if (tid == 0) {
        a.motion[3 * b] = m.a;
        a.motion[3 * b + 1] = m.b0;
        a.motion[3 * b + 2] = m.b1;
        a.count[b] = (int32_t)sr[1];
        a.rms[b] = failed ? qnan : sqrt(sr[0] / m.W);
        a.ok[b] = failed ? 0 : 1;
    }
}

__global__ void pose_advance_kernel(const double *motion, const uint8_t *ok, double *pose, float *rot, double *trans,
                                    double *flow_trans, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double x0 = pose[3 * b], y0 = pose[3 * b + 1], phi0 = pose[3 * b + 2];
    double x1 = x0, y1 = y0, phi1 = phi0, dx = 0.0, dy = 0.0;
    if (ok[b]) {
        const double theta = motion[3 * b], ux = motion[3 * b + 1], uy = motion[3 * b + 2];
        double s0, c0;
        sincos(phi0, &s0, &c0);
        phi1 = phi0 + theta;
        x1 = x0 + (c0 * ux - s0 * uy);
        y1 = y0 + (s0 * ux + c0 * uy);
        dx = x1 - x0;
        dy = y1 - y0;
    }
    pose[3 * b] = x1;
    pose[3 * b + 1] = y1;
    pose[3 * b + 2] = phi1;
    pof_write_pose_terms(b, x1, y1, phi1, dx, dy, rot, trans, flow_trans);
}

}  // namespace

extern "C" int pof_ego_motion(const float *ranges, const double *xy, const double *tab, const void *flow, int flow_f64,
                              int canonical, int sign, int model, const float *weight, const int32_t *instance_mask,
                              const int32_t *num_det, const double *det_cls, double cls_thresh, double max_range,
                              double huber_delta, int iters, int B, int N, double *motion, int32_t *count,
                              double *rms, uint8_t *ok, double *flow_residual, float *weight_out, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if ((!ranges && !xy) || !flow || !motion || !count || !rms || !ok) return POF_E_BADARG;
    if (!tab && (canonical || !xy)) return POF_E_BADARG;       // the table rotates the flow and places the ranges
    if ((sign != 1 && sign != -1) || (model != 0 && model != 1) || iters < 0 || iters > kMaxIters)
        return POF_E_BADARG;
    if (instance_mask && (!num_det || !det_cls)) return POF_E_BADARG;
    if (B < 0 || N < 1) return POF_E_BADARG;
    if (N > kGroupMaxN) return POF_E_SHAPE;                    // the limit of pof_nms_predicted_center
    if (B == 0) return POF_OK;
    EgoMotionArgs a;
    a.ranges = ranges; a.xy = xy; a.tab = tab; a.flow = flow; a.weight = weight;
    a.gate = {instance_mask, num_det, det_cls, cls_thresh}; a.max_range = max_range;
    a.huber_delta = huber_delta; a.flow_f64 = flow_f64; a.canonical = canonical; a.sign = sign; a.model = model;
    a.iters = iters; a.N = N; a.motion = motion; a.count = count; a.rms = rms; a.ok = ok;
    a.flow_residual = flow_residual; a.weight_out = weight_out;
    POF_LAUNCH_PER_SENSOR(ego_motion_kernel, N, B, stream, a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}

extern "C" int pof_pose_advance(const double *motion, const uint8_t *ok, double *pose, float *rot, double *trans,
                                double *flow_trans, int B, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!motion || !ok || !pose) return POF_E_BADARG;
    if (B < 0) return POF_E_BADARG;
    if (B == 0) return POF_OK;
    pose_advance_kernel<<<(B + 63) / 64, 64, 0, pof_stream(stream)>>>(motion, ok, pose, rot, trans, flow_trans, B);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
