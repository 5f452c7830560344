// A11: nms_predicted_center (src/utils/utils.py:535-571), one workgroup per scan.
//
//   1. regression offsets -> detection centres (canonical_to_global + rphi_to_xy)
//   2. sort by descending score (bitonic, in LDS).  The order is total: equal scores (a saturated
//      sigmoid gives many exact 1.0s in deployment) are visited by DESCENDING point index, i.e. like
//      np.argsort(kind="stable")[::-1]; the reference's argsort()[::-1] leaves ties to NumPy's
//      introsort, so only distinct scores are comparable with it bit for bit
//   3. greedy suppression in score order: a kept centre labels every centre
//      closer than min_dist with its instance id (later ids overwrite earlier
//      ones, as in the reference) and suppresses it
//   4. kept centres compacted in score order.
// Serial in the number of kept centres and latency bound: reported in
// microseconds, not GB/s.
//
// Round 3, N <= 512 (nms_wave_kernel): ONE WAVE PER SCAN, no workgroup barrier anywhere.
//   * lane l owns the sorted positions l, l + 64, ...: up to 8 columns, their centres in registers;
//   * order: a bitonic network over (score, point index) in LDS in its all-ascending form (the padding to a
//     power of two is virtual), 45 steps of 4 compare-exchanges per lane for N = 450;
//   * the greedy walk visits KEPT centres only: the alive set is eight 64-bit ballots in scalar registers, the
//     next kept index is a count-trailing-zeros; its row of the suppression relation is evaluated on demand by
//     the 64 lanes (8 exact float64 distance tests each -- no square root: sqrt is monotone and correctly rounded,
//     so RN(sqrt(s)) < min_dist  <=>  s <= s*, the largest float64 with that property, found on the host with
//     nextafter) and applied with ballots; the lanes keep the instance id of their columns in registers (later
//     kept centres overwrite earlier labels, as in the reference);
//   * round 2's kernel paid two workgroup barriers per POINT (450 x 2 per scan), kept or not: 0.26 ms for 1024
//     scans; an intermediate round-3 form that built the whole N x N relation up front did four times the distance
//     tests the walk needs and measured 0.38 ms.
#include <cmath>

#include "pof_common.h"

namespace {

constexpr int kThreads = 512;

struct NmsArgs {
    const float *ranges;
    const double *tab;
    const double *pred_cls;
    const double *pred_reg;
    double min_dist;
    int N, Npad;
    double *det_xy, *det_cls;
    int32_t *num_det, *instance_mask;
};

__global__ __launch_bounds__(kThreads) void nms_kernel(NmsArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int N = a.N, Np = a.Npad;
    double *s_key = reinterpret_cast<double *>(smem);  // score, sorted descending
    double *s_x = s_key + Np;
    double *s_y = s_x + Np;
    int *s_ord = reinterpret_cast<int *>(s_y + Np);    // original point index
    int *s_keep = s_ord + Np;
    int *s_scan = s_keep + Np;
    __shared__ int s_flag;

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const float *r = a.ranges + (long long)b * N;
    const double *cls = a.pred_cls + (long long)b * N;
    const double *reg = a.pred_reg + (long long)b * N * 2;

    for (int i = tid; i < Np; i += kThreads) {
        if (i < N) {
            s_key[i] = cls[i];
            s_ord[i] = i;
        } else {
            s_key[i] = -INFINITY;  // padding sorts to the end
            s_ord[i] = -1;
        }
    }
    __syncthreads();
    // bitonic sort, descending by key
    for (int k = 2; k <= Np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < Np; i += kThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const bool desc = (i & k) == 0;
                    const double ki = s_key[i], kl = s_key[l];
                    const int oi = s_ord[i], ol = s_ord[l];
                    // total order: (score, point index) descending; padding (-inf, ord -1) stays behind
                    // real entries
                    const bool l_first = (kl > ki) || (kl == ki && ol > oi);
                    const bool i_first = (ki > kl) || (ki == kl && oi > ol);
                    const bool swap = desc ? l_first : i_first;
                    if (swap) {
                        s_key[i] = kl;
                        s_key[l] = ki;
                        s_ord[i] = ol;
                        s_ord[l] = oi;
                    }
                }
            }
            __syncthreads();
        }
    }
    // centres in sorted order
    for (int i = tid; i < Np; i += kThreads) {
        if (i < N) {
            const int src = s_ord[i];
            const double ty = (double)r[src] + reg[2 * src + 1];
            const double tphi = atan2(reg[2 * src], ty);
            const double dphi = tphi + a.tab[src];
            const double dr = ty / cos(tphi);
            double s, c;
            sincos(dphi, &s, &c);
            s_x[i] = dr * c;
            s_y[i] = dr * s;
            s_keep[i] = 1;
        } else {
            s_keep[i] = 0;
        }
    }
    int32_t *inst = a.instance_mask + (long long)b * N;
    for (int i = tid; i < N; i += kThreads) inst[i] = 0;
    __syncthreads();

    int next_id = 1;
    for (int i = 0; i < N; ++i) {
        if (tid == 0) s_flag = s_keep[i];
        __syncthreads();
        const int live = s_flag;
        if (live) {
            const double xi = s_x[i], yi = s_y[i];
            for (int j = tid; j < N; j += kThreads) {
                const double dx = xi - s_x[j], dy = yi - s_y[j];
                const double dist = sqrt(dx * dx + dy * dy);
                if (dist < a.min_dist) {
                    s_keep[j] = (j == i);
                    inst[s_ord[j]] = next_id;
                }
            }
            ++next_id;
        }
        __syncthreads();
    }

    // compaction of kept centres (inclusive Hillis-Steele scan over Npad flags)
    for (int i = tid; i < Np; i += kThreads) s_scan[i] = s_keep[i];
    __syncthreads();
    for (int off = 1; off < Np; off <<= 1) {
        int v[8];
        int cnt = 0;
        for (int i = tid; i < Np; i += kThreads) v[cnt++] = (i >= off) ? s_scan[i - off] : 0;
        __syncthreads();
        cnt = 0;
        for (int i = tid; i < Np; i += kThreads) s_scan[i] += v[cnt++];
        __syncthreads();
    }
    double *oxy = a.det_xy + (long long)b * N * 2;
    double *ocl = a.det_cls + (long long)b * N;
    for (int i = tid; i < N; i += kThreads) {
        if (s_keep[i]) {
            const int pos = s_scan[i] - 1;
            oxy[2 * pos] = s_x[i];
            oxy[2 * pos + 1] = s_y[i];
            ocl[pos] = s_key[i];
        }
    }
    if (tid == 0) a.num_det[b] = s_scan[Np - 1];
}

constexpr int kSmallMaxN = 512;
constexpr int kCols = kSmallMaxN / 64;      // sorted positions per lane

struct NmsSmallArgs {
    NmsArgs a;
    double s2_thr;      // dist < min_dist  <=>  dx*dx + dy*dy <= s2_thr
};

__global__ __launch_bounds__(64) void nms_wave_kernel(NmsSmallArgs A)
{
    __shared__ double s_key[kSmallMaxN];     // score, sorted
    __shared__ double s_x[kSmallMaxN], s_y[kSmallMaxN];
    __shared__ int s_ord[kSmallMaxN];        // point index of a sorted position
    __shared__ int s_kept[kSmallMaxN];       // sorted positions of the kept centres, in order
    const NmsArgs &a = A.a;
    const int N = a.N, b = blockIdx.x, lane = threadIdx.x;
    const float *r = a.ranges + (long long)b * N;
    const double *cls = a.pred_cls + (long long)b * N;
    const double *reg = a.pred_reg + (long long)b * N * 2;
    for (int i = lane; i < N; i += 64) {
        s_key[i] = cls[i];
        s_ord[i] = i;
    }
    pof_lds_order<64>();
    // bitonic network, all-ascending form, on the total order "u comes before v": (score, point index)
    // descending; a NaN score comes after every number (NumPy sorts NaNs to the end of the ascending order, the
    // reference reverses it -- its NaNs lead; either way the order among NaNs is by point index and a scan with
    // NaN scores is not a comparable case)
    int npad = 1;
    while (npad < N) npad <<= 1;
    const int half = npad >> 1;
    auto cmpx = [&](int lo, int hi) {
        if (hi < N) {
            const double kl = s_key[lo], kh = s_key[hi];
            const int ol = s_ord[lo], oh = s_ord[hi];
            const bool nl = kl != kl, nh = kh != kh;
            const bool hi_first = (!nh && nl) || (nl == nh && ((kh > kl) || (!(kl > kh) && oh > ol)));
            if (hi_first) {
                s_key[lo] = kh;
                s_key[hi] = kl;
                s_ord[lo] = oh;
                s_ord[hi] = ol;
            }
        }
    };
    for (int k = 2; k <= npad; k <<= 1) {
        const int hk = k >> 1;
        for (int t = lane; t < half; t += 64) {
            const int blk = t / hk, off = t - blk * hk;
            cmpx(blk * k + off, blk * k + k - 1 - off);
        }
        pof_lds_order<64>();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int t = lane; t < half; t += 64) {
                const int lo = 2 * j * (t / j) + (t % j);
                cmpx(lo, lo + j);
            }
            pof_lds_order<64>();
        }
    }
    // centres of this lane's columns (sorted positions lane + 64 c)
    double xr[kCols], yr[kCols];
    int inst_id[kCols];
    unsigned long long alive[kCols];         // wave-uniform ballots: column c of lane l alive <=> bit l
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        const int i = lane + 64 * c;
        xr[c] = yr[c] = 0.0;
        inst_id[c] = 0;
        if (i < N) {
            const int src = s_ord[i];
            const double ty = (double)r[src] + reg[2 * src + 1];
            const double tphi = atan2(reg[2 * src], ty);
            const double dphi = tphi + a.tab[src];
            const double dr = ty / cos(tphi);
            double sn, cs;
            sincos(dphi, &sn, &cs);
            xr[c] = dr * cs;
            yr[c] = dr * sn;
            s_x[i] = xr[c];
            s_y[i] = yr[c];
        }
        alive[c] = __ballot(i < N);
    }
    pof_lds_order<64>();
    // greedy walk over the kept centres
    int nkept = 0;
    while (true) {
        int i = -1;
#pragma unroll
        for (int c = kCols - 1; c >= 0; --c)
            if (alive[c] != 0ull) i = 64 * c + __builtin_ctzll(alive[c]);
        if (i < 0) break;
        const double xi = s_x[i], yi = s_y[i];
        ++nkept;
        if (lane == 0) s_kept[nkept - 1] = i;
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const double dx = xi - xr[c], dy = yi - yr[c];
            const bool hit = (lane + 64 * c < N) && (dx * dx + dy * dy <= A.s2_thr);
            alive[c] &= ~__ballot(hit);
            if (hit) inst_id[c] = nkept;
            // the kept centre leaves the set even when it is not within min_dist of itself (NaN centre)
            if ((i >> 6) == c) alive[c] &= ~(1ull << (i & 63));
        }
    }
    pof_lds_order<64>();
    int32_t *inst = a.instance_mask + (long long)b * N;
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        const int i = lane + 64 * c;
        if (i < N) inst[s_ord[i]] = inst_id[c];
    }
    double *oxy = a.det_xy + (long long)b * N * 2;
    double *ocl = a.det_cls + (long long)b * N;
    for (int k = lane; k < nkept; k += 64) {
        const int i = s_kept[k];
        oxy[2 * k] = s_x[i];
        oxy[2 * k + 1] = s_y[i];
        ocl[k] = s_key[i];
    }
    if (lane == 0) a.num_det[b] = nkept;
}

// largest float64 s with RN(sqrt(s)) < r (the reference compares the rounded distance with min_dist)
double nms_sq_threshold(double r)
{
    if (!(r > 0.0)) return -1.0;
    double c = r * r;
    for (int it = 0; it < 64 && !(std::sqrt(c) < r); ++it) c = std::nextafter(c, 0.0);
    for (int it = 0; it < 64; ++it) {
        const double up = std::nextafter(c, HUGE_VAL);
        if (!(std::sqrt(up) < r)) break;
        c = up;
    }
    return c;
}

int next_pow2(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

extern "C" size_t pof_nms_workspace_bytes(int B, int N)
{
    (void)B;
    (void)N;
    return 0;  // everything lives in LDS; kept in the ABI for larger scans
}

extern "C" int pof_nms_predicted_center(const float *ranges, const double *tab, const double *pred_cls,
                                        const double *pred_reg, double min_dist, int B, int N,
                                        double *det_xy, double *det_cls, int32_t *num_det,
                                        int32_t *instance_mask, void *workspace, size_t workspace_bytes,
                                        pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    (void)workspace;
    (void)workspace_bytes;
    if (!ranges || !tab || !pred_cls || !pred_reg || !det_xy || !det_cls || !num_det || !instance_mask)
        return POF_E_BADARG;
    if (B < 0 || N < 1) return POF_E_BADARG;
    if (B == 0) return POF_OK;
    NmsArgs a;
    a.ranges = ranges; a.tab = tab; a.pred_cls = pred_cls; a.pred_reg = pred_reg; a.min_dist = min_dist;
    a.N = N; a.Npad = next_pow2(N);
    a.det_xy = det_xy; a.det_cls = det_cls; a.num_det = num_det; a.instance_mask = instance_mask;
    if (N <= kSmallMaxN && std::isfinite(min_dist)) {
        NmsSmallArgs A;
        A.a = a;
        A.s2_thr = nms_sq_threshold(min_dist);
        nms_wave_kernel<<<B, 64, 0, pof_stream(stream)>>>(A);
        POF_CHECK_LAUNCH();
        return POF_OK;
    }
    if (a.Npad > 4096) return POF_E_SHAPE;  // 8 flags per thread in the scan
    a.det_xy = det_xy; a.det_cls = det_cls; a.num_det = num_det; a.instance_mask = instance_mask;
    const size_t lds = (size_t)a.Npad * (3 * sizeof(double) + 3 * sizeof(int));
    if (lds > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(nms_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return POF_E_LAUNCH;
    }
    nms_kernel<<<B, kThreads, lds, pof_stream(stream)>>>(a);
    POF_CHECK_LAUNCH();
    return POF_OK;
}
