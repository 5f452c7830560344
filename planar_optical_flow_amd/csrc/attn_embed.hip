// A10, the attention gate's embedding (src/depracted/model/dr_spaam.py:137-147, :166-171): Conv1d(n_channel -> E,
// kernel_size = n_pts) + BatchNorm1d(eval) + LeakyReLU on [.., n_channel, n_pts] cutout features.  The kernel spans
// the whole cutout, so it is the dense product
//
//   emb[r][e] = lrelu( sum_k src[r][k] * w[e][k] + bias[e] ),   src in {x, tmpl},  K = n_channel * n_pts
//
// with the BatchNorm folded into w / bias (fold_for_inference).  Both sources go in ONE launch (blockIdx.z) and share
// w; rows are float32 or float16 (storage type T, widened in front of the MFMA -- exact), every product and sum is
// float32 on v_mfma_f32_32x32x2_f32.  No workspace, no memset, no atomics.
//
// SUMMATION ORDER -- one order for every R, both storage types and both kernel forms:
//   * k is cut into chunks of 8; chunk c belongs to chain c % 4;
//   * a chain starts at +0.0f and takes its chunks in ascending order; inside a chunk it takes k in the order
//     8c+0, 8c+4, 8c+1, 8c+5, 8c+2, 8c+6, 8c+3, 8c+7, each step p = fmaf(src[r][k], w[e][k], p)
//     (four MFMAs per chunk, MFMA j holds the k-pair {8c + j, 8c + 4 + j}; on gfx950 the float32-input MFMA is
//     bit for bit that k-ordered fmaf chain);
//   * s = ((p0 + p1) + p2) + p3;  v = s + bias[e];  emb = v >= 0 ? v : v * (float)negative_slope.
//
// Operands as in dense_small.hip: both are K-contiguous, lane (r, h) of the A operand holds src[row0 + r][8c + 4h ..
// + 3], of the B operand w[e0 + r][same k] -- 16 bytes of its row per chunk (8 bytes of a float16 row).
//
// Two forms, same bits (pof_attn_embed_plan):
//   form 0 (R < kEmbLargeRows): one workgroup per 32 x 32 output tile; its four waves ARE the four chains (wave =
//     chain), they meet in LDS and wave 0 adds them in chain order.  R = 450, E = 128, two sources: 120 workgroups of
//     four busy SIMDs.
//   form 1 (R >= kEmbLargeRows): one workgroup per 64 rows x 128 columns, one wave per 64 x 32: it carries the four
//     chains of its two row tiles as eight independent accumulators (the MFMA's 64-cycle dependent latency is
//     covered by its own issue) and reads every w element once per 64 rows instead of once per 32.
// Rows past R in a ragged tile read a clamped valid row; their results are not stored.
#include "pof_common.h"

namespace {

using f32x16 = float __attribute__((ext_vector_type(16)));
using F4V = float __attribute__((ext_vector_type(4)));
using H4V = _Float16 __attribute__((ext_vector_type(4)));
constexpr int kEmbChains = 4;
constexpr int kEmbAhead = 4;             // form 0: chunks of loads in flight per wave
constexpr long long kEmbLargeRows = 8192;   // form 1 from this many rows per source

template <typename T> struct EmbArgs {
    const T *src[2];
    float *emb[2];
    const float *w, *bias;
    long long R;
    int K, E;
    float slope;
};

__device__ __forceinline__ F4V emb_load4(const float *p) { return *reinterpret_cast<const F4V *>(p); }
__device__ __forceinline__ F4V emb_load4(const _Float16 *p)
{
    const H4V v = *reinterpret_cast<const H4V *>(p);
    return F4V{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// bias, LeakyReLU and the store of one lane's 16 results of a 32 x 32 tile (C/D layout: column = lane & 31,
// row = (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5))
__device__ __forceinline__ void emb_store(float *emb, long long row0, long long R, int E, int e, int h, float bias,
                                          float slope, const f32x16 &s)
{
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const long long row = row0 + (v & 3) + 8 * (v >> 2) + 4 * h;
        const float y = s[v] + bias;
        if (row < R) emb[row * E + e] = y >= 0.0f ? y : y * slope;
    }
}

// form 0: wave = chain
template <typename T> __global__ __launch_bounds__(64 * kEmbChains) void attn_embed_split_kernel(EmbArgs<T> a)
{
    __shared__ float s_acc[kEmbChains - 1][16][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long long row0 = (long long)blockIdx.x * 32;
    const int e0 = blockIdx.y * 32;
    const T *px = a.src[blockIdx.z] + min(row0 + r, a.R - 1) * a.K + 4 * h;
    const float *pw = a.w + (long long)(e0 + r) * a.K + 4 * h;
    const int nchunk = a.K >> 3;
    f32x16 acc = f32x16{0};
    for (int c0 = wave; c0 < nchunk; c0 += kEmbChains * kEmbAhead) {
        F4V va[kEmbAhead], vb[kEmbAhead];
#pragma unroll
        for (int u = 0; u < kEmbAhead; ++u) {
            const int c = c0 + u * kEmbChains;
            const bool ok = c < nchunk;
            va[u] = ok ? emb_load4(px + 8 * c) : F4V{0.0f, 0.0f, 0.0f, 0.0f};
            vb[u] = ok ? emb_load4(pw + 8 * c) : F4V{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int u = 0; u < kEmbAhead; ++u) {
            if (c0 + u * kEmbChains >= nchunk) break;      // wave-uniform: a chain ends with its last chunk, no +0 steps
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[u][j], vb[u][j], acc, 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) s_acc[wave - 1][v][lane] = acc[v];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < kEmbChains - 1; ++w)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] += s_acc[w][v][lane];
    emb_store(a.emb[blockIdx.z], row0, a.R, a.E, e0 + r, h, a.bias[e0 + r], a.slope, acc);
}

// form 1: one wave per 64 rows x 32 columns, the four chains of both row tiles in registers
template <typename T> __global__ __launch_bounds__(256, 2) void attn_embed_wide_kernel(EmbArgs<T> a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long long row0 = (long long)blockIdx.x * 64;
    const int e0 = (blockIdx.y * 4 + wave) * 32;
    if (e0 >= a.E) return;                                  // E < 128: the spare waves leave (no barrier below)
    const T *px0 = a.src[blockIdx.z] + min(row0 + r, a.R - 1) * a.K + 4 * h;
    const T *px1 = a.src[blockIdx.z] + min(row0 + 32 + r, a.R - 1) * a.K + 4 * h;
    const float *pw = a.w + (long long)(e0 + r) * a.K + 4 * h;
    const int nchunk = a.K >> 3;
    f32x16 acc0[kEmbChains], acc1[kEmbChains];
#pragma unroll
    for (int q = 0; q < kEmbChains; ++q) acc0[q] = acc1[q] = f32x16{0};
    // chunks 4g .. 4g + 3 feed chains 0 .. 3; the next group's loads are issued before this group's MFMAs
    F4V xa[kEmbChains], xb[kEmbChains], wv[kEmbChains];
    const int ngroup = nchunk >> 2;
    if (ngroup > 0) {
#pragma unroll
        for (int q = 0; q < kEmbChains; ++q) {
            xa[q] = emb_load4(px0 + 8 * q);
            xb[q] = emb_load4(px1 + 8 * q);
            wv[q] = emb_load4(pw + 8 * q);
        }
    }
    for (int g = 0; g < ngroup; ++g) {
        F4V na[kEmbChains], nb[kEmbChains], nw[kEmbChains];
        const int cn = min(g + 1, ngroup - 1) * 4;          // the last group re-reads itself (in bounds, unused)
#pragma unroll
        for (int q = 0; q < kEmbChains; ++q) {
            na[q] = emb_load4(px0 + 8 * (cn + q));
            nb[q] = emb_load4(px1 + 8 * (cn + q));
            nw[q] = emb_load4(pw + 8 * (cn + q));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < kEmbChains; ++q) {
                acc0[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[q][j], wv[q][j], acc0[q], 0, 0, 0);
                acc1[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[q][j], wv[q][j], acc1[q], 0, 0, 0);
            }
#pragma unroll
        for (int q = 0; q < kEmbChains; ++q) {
            xa[q] = na[q];
            xb[q] = nb[q];
            wv[q] = nw[q];
        }
    }
    // the ragged last group: K / 8 is no multiple of four, chains 0 .. rem - 1 take one more chunk
    const int rem = nchunk & 3;
#pragma unroll
    for (int q = 0; q < kEmbChains - 1; ++q) {
        if (q < rem) {
            const int c = ngroup * 4 + q;
            const F4V ta = emb_load4(px0 + 8 * c), tb = emb_load4(px1 + 8 * c), tw = emb_load4(pw + 8 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[j], tw[j], acc0[q], 0, 0, 0);
                acc1[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(tb[j], tw[j], acc1[q], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int q = 1; q < kEmbChains; ++q)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            acc0[0][v] += acc0[q][v];
            acc1[0][v] += acc1[q][v];
        }
    const float bias = a.bias[e0 + r];
    emb_store(a.emb[blockIdx.z], row0, a.R, a.E, e0 + r, h, bias, a.slope, acc0[0]);
    emb_store(a.emb[blockIdx.z], row0 + 32, a.R, a.E, e0 + r, h, bias, a.slope, acc1[0]);
}

int emb_check_shape(long long R, int K, int E)
{
    if (R < 1 || K < 1 || E < 1) return POF_E_BADARG;
    if ((K & 7) || (E & 31) || E < 32 || E > 256) return POF_E_SHAPE;
    if ((R + 31) / 32 > 0x7fffffffLL) return POF_E_SHAPE;
    return POF_OK;
}

int emb_form(long long R) { return R >= kEmbLargeRows ? 1 : 0; }

template <typename T>
int emb_launch(const T *x, const T *tmpl, long long R, int K, int E, const float *w, const float *bias,
               double negative_slope, float *emb_x, float *emb_t, pof_stream_t stream)
{
    POF_CLEAR_STALE_ERROR();
    if (!x || !w || !bias || !emb_x) return POF_E_BADARG;
    if ((tmpl == nullptr) != (emb_t == nullptr)) return POF_E_BADARG;
    const int rc = emb_check_shape(R, K, E);
    if (rc != POF_OK) return rc;
    const uintptr_t bases = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(tmpl) |
                            reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(emb_x) |
                            reinterpret_cast<uintptr_t>(emb_t);
    if (bases & 15) return POF_E_SHAPE;
    EmbArgs<T> a{{x, tmpl}, {emb_x, emb_t}, w, bias, R, K, E, (float)negative_slope};
    const unsigned nsrc = tmpl ? 2u : 1u;
    if (emb_form(R) == 0) {
        const dim3 grid((unsigned)((R + 31) / 32), (unsigned)(E / 32), nsrc);
        attn_embed_split_kernel<T><<<grid, 64 * kEmbChains, 0, pof_stream(stream)>>>(a);
    } else {
        const dim3 grid((unsigned)((R + 63) / 64), (unsigned)((E + 127) / 128), nsrc);
        attn_embed_wide_kernel<T><<<grid, 256, 0, pof_stream(stream)>>>(a);
    }
    POF_CHECK_LAUNCH();
    return POF_OK;
}

}  // namespace

extern "C" int pof_attn_embed(const float *x, const float *tmpl, long long R, int K, int E, const float *w,
                              const float *bias, double negative_slope, float *emb_x, float *emb_t,
                              pof_stream_t stream)
{
    return emb_launch<float>(x, tmpl, R, K, E, w, bias, negative_slope, emb_x, emb_t, stream);
}

extern "C" int pof_attn_embed_f16(const void *x_f16, const void *tmpl_f16, long long R, int K, int E, const float *w,
                                  const float *bias, double negative_slope, float *emb_x, float *emb_t,
                                  pof_stream_t stream)
{
    return emb_launch<_Float16>(static_cast<const _Float16 *>(x_f16), static_cast<const _Float16 *>(tmpl_f16), R, K, E,
                                w, bias, negative_slope, emb_x, emb_t, stream);
}

extern "C" int pof_attn_embed_plan(long long R, int K, int E, int *form)
{
    if (!form) return POF_E_BADARG;
    const int rc = emb_check_shape(R, K, E);
    if (rc != POF_OK) return rc;
    *form = emb_form(R);
    return POF_OK;
}
