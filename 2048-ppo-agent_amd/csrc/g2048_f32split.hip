// Reference-precision (f32-grade) rollout forward of the default-shape PPOAgent on the f16 matrix cores.
//
// The reference rolls out in fp32 (src/ppo/torch_action_wrapper.py:73-102).  A Linear y = x W^T is computed here as a two-way fp16
// split product: x = (hi_x + lo_x) / sx, w = (hi_w + lo_w) / sw with hi = f16(s v), lo = f16(s v - hi) (11 + 11 significand bits),
// three v_mfma_f32_32x32x16_f16 per fragment pair (lo_w hi_x, hi_w lo_x, hi_w hi_x) into ONE f32 accumulator, the dropped lo lo term
// being 2^-22 relative; the epilogue multiplies by 1 / (sx sw) in f32.  sx and sw are powers of two (exact), chosen by the caller
// so that every operand keeps |s v| <= 2^15 (hi finite): an operand beyond that turns into inf / NaN in the output, never into a
// quietly wrong number.  Elements with |s v| >= 2^-3 keep both halves in fp16's NORMAL range; below that their absolute error is at
// most 2^-14 / s (lo flushed) whatever the matrix core does with fp16 subnormals.  src/ppo/fused_policy.py (FusedPolicyF32) derives
// the scales from bounds that hold for every input, see DESIGN.md.
//
// Kernels: k_split_pack (weights -> hi / lo planes in fragment order), k_split_gemm<EPI> (the GEMM with its epilogues),
// k_attn17_f32 (17-token attention on the packed f32 in_proj output: k_attn_fwd17 of g2048_attention.hip with f32 I/O, no dropout),
// k_embed_ln_f32 (embedding + positions + CLS row + the first LayerNorm, all f32).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_mfma.h"

namespace {

using namespace g2048_mfma;
using namespace g2048_host;

// ------------------------------------------------------------------------------------------------ weight pack
// packed[(((c KS + ks) 8 + nt) 2 + p) 64 + l][j] = plane p of w[256 c + 32 nt + (l & 31)][16 ks + 8 (l >> 5) + j]: the A fragment of
// lane l for output tile nt of column chunk c at k-step ks (f16x8 units; KS = K / 16).  One (c, ks) block is 16 KB, contiguous.
__global__ void __launch_bounds__(256) k_split_pack(const float *__restrict__ w, int N, int K, float s, f16x8 *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one (n, group of 8 k) each
    if (idx >= (int64_t)N * (K / 8)) return;
    const int n = (int)(idx / (K / 8)), k8 = (int)(idx % (K / 8));
    f16x8 hi, lo;
    float wv[8];
    for (int j = 0; j < 8; ++j) wv[j] = w[(size_t)n * K + 8 * k8 + j];
    split_f16(wv, s, hi, lo);
    const int c = n >> 8, nt = (n >> 5) & 7, r = n & 31, ks = k8 >> 1, h = k8 & 1;
    const size_t o = ((((size_t)c * (K / 16) + ks) * 8 + nt) * 2) * 64 + (32 * h + r);
    out[o] = hi;
    out[o + 64] = lo;
}

// ------------------------------------------------------------------------------------------------ the GEMM
// Workgroup: 128 tokens x 256 outputs (column chunk blockIdx.y), 4 waves of 32 tokens x 256 outputs (8 accumulator tiles: a token's
// 256 outputs sit in the two lanes r and r + 32, so LayerNorm's row statistics are in-lane sums plus one exchange).  Tokens are the B
// operand, read straight from global memory (each lane its own 32 bytes per k-step: every byte of X is read once per column chunk) and
// split in registers; the weight block of a k-step (16 KB) goes global -> registers -> LDS one step ahead, double-buffered, one
// barrier per step.
template <int EPI>
__global__ void __launch_bounds__(256, 2)
k_split_gemm(const float *__restrict__ X, int64_t ldx, const f16x8 *__restrict__ Wp, const float *__restrict__ bias, float *Y, int64_t ldy,
             const float *resid, const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ Hn, int64_t T, int K,
             float sx, float inv, float eps) {
    __shared__ f16x8 lds[2][1024];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t tok = (int64_t)blockIdx.x * 128 + 32 * wv + r;
    const int64_t tokc = tok < T ? tok : T - 1;  // rows past T read the last row and store nothing
    const float *xp = X + tokc * ldx + 8 * h;
    const int nks = K >> 4;
    const f16x8 *wp = Wp + (size_t)blockIdx.y * nks * 1024 + tid;
    f32x16 acc[8];
    for (int nt = 0; nt < 8; ++nt) acc[nt] = zero_tile();
    f16x8 st[4];
    for (int i = 0; i < 4; ++i) st[i] = wp[256 * i];
    float4 xa = *reinterpret_cast<const float4 *>(xp), xb = *reinterpret_cast<const float4 *>(xp + 4);
    for (int i = 0; i < 4; ++i) lds[0][tid + 256 * i] = st[i];
    __syncthreads();
    for (int ks = 0; ks < nks; ++ks) {
        f16x8 hi, lo;
        const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
        split_f16(xv, sx, hi, lo);
        const bool more = ks + 1 < nks;
        if (more) {
            for (int i = 0; i < 4; ++i) st[i] = wp[(size_t)(ks + 1) * 1024 + 256 * i];
            xa = *reinterpret_cast<const float4 *>(xp + 16 * (ks + 1));
            xb = *reinterpret_cast<const float4 *>(xp + 16 * (ks + 1) + 4);
        }
        const f16x8 *L = lds[ks & 1] + lane;
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // four tiles at a time: 12 MFMAs on four independent accumulators
            f16x8 whi[4], wlo[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                whi[i] = L[(8 * q + 2 * i) * 64];
                wlo[i] = L[(8 * q + 2 * i + 1) * 64];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[4 * q + i] = mfma_f16(wlo[i], hi, acc[4 * q + i]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[4 * q + i] = mfma_f16(whi[i], lo, acc[4 * q + i]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[4 * q + i] = mfma_f16(whi[i], hi, acc[4 * q + i]);
        }
        if (more)
            for (int i = 0; i < 4; ++i) lds[(ks + 1) & 1][tid + 256 * i] = st[i];
        __syncthreads();
    }
    // ---- epilogue: acc[nt][4 g + q] is output 32 nt + 8 g + 4 h + q of this lane's token
    const bool live = tok < T;
    const int n0 = 256 * blockIdx.y;
    if constexpr (EPI == G2048_F32SPLIT_BIAS || EPI == G2048_F32SPLIT_BIAS_RELU) {
        float *yp = Y + tokc * ldy + n0;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = 32 * nt + 8 * g + 4 * h;
                const float4 b = *reinterpret_cast<const float4 *>(bias + n0 + n);
                float4 v = make_float4(acc[nt][4 * g] * inv + b.x, acc[nt][4 * g + 1] * inv + b.y, acc[nt][4 * g + 2] * inv + b.z,
                                       acc[nt][4 * g + 3] * inv + b.w);
                if constexpr (EPI == G2048_F32SPLIT_BIAS_RELU) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
                if (live) *reinterpret_cast<float4 *>(yp + n) = v;
            }
    } else {
        // residual stream out (Y may be resid itself: every element is read by the lane that writes it), then LayerNorm of the row
        const float *rp = resid + tokc * 256;
        float *yp = Y + tokc * ldy;
        float sum = 0.f;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = 32 * nt + 8 * g + 4 * h;
                const float4 b = *reinterpret_cast<const float4 *>(bias + n), x0 = *reinterpret_cast<const float4 *>(rp + n);
                const float4 v = make_float4(x0.x + (acc[nt][4 * g] * inv + b.x), x0.y + (acc[nt][4 * g + 1] * inv + b.y),
                                             x0.z + (acc[nt][4 * g + 2] * inv + b.z), x0.w + (acc[nt][4 * g + 3] * inv + b.w));
                if (live) *reinterpret_cast<float4 *>(yp + n) = v;
                acc[nt][4 * g] = v.x; acc[nt][4 * g + 1] = v.y; acc[nt][4 * g + 2] = v.z; acc[nt][4 * g + 3] = v.w;
                sum += (v.x + v.y) + (v.z + v.w);
            }
        if constexpr (EPI == G2048_F32SPLIT_ADD_LN) {
            sum += __shfl_xor(sum, 32);
            const float mean = sum * (1.0f / 256.0f);
            float ss = 0.f;
#pragma unroll
            for (int nt = 0; nt < 8; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float d = acc[nt][i] - mean;
                    ss = fmaf(d, d, ss);
                }
            ss += __shfl_xor(ss, 32);
            const float rstd = 1.0f / sqrtf(ss * (1.0f / 256.0f) + eps);
            float *hp = Hn + tokc * 256;
#pragma unroll
            for (int nt = 0; nt < 8; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = 32 * nt + 8 * g + 4 * h;
                    const float4 ga = *reinterpret_cast<const float4 *>(gamma + n), be = *reinterpret_cast<const float4 *>(beta + n);
                    const float4 v = make_float4((acc[nt][4 * g] - mean) * rstd * ga.x + be.x, (acc[nt][4 * g + 1] - mean) * rstd * ga.y + be.y,
                                                 (acc[nt][4 * g + 2] - mean) * rstd * ga.z + be.z, (acc[nt][4 * g + 3] - mean) * rstd * ga.w + be.w);
                    if (live) *reinterpret_cast<float4 *>(hp + n) = v;
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ attention, 17 tokens, f32
// One lane per query row, 3 (sample, head) pairs per wavefront, K and V rows in LDS: k_attn_fwd17 with f32 I/O, precise expf, no
// dropout.  qkv f32 [B][17][3 * 32 H] (the packed in_proj output, read in place), o f32 [B][17][32 H].
constexpr int HD = 32, SK = 17, PAIRS = 3, ROW = HD + 4, PSTRIDE = SK * ROW + 8;

__device__ __forceinline__ void load_row_f32(const float *p, float out[HD]) {
    for (int c = 0; c < HD / 4; ++c) {
        const float4 u = *reinterpret_cast<const float4 *>(p + 4 * c);
        out[4 * c] = u.x; out[4 * c + 1] = u.y; out[4 * c + 2] = u.z; out[4 * c + 3] = u.w;
    }
}
__device__ __forceinline__ void put_row_f32(float *row, const float v[HD]) {
    for (int c = 0; c < HD / 4; ++c) *reinterpret_cast<float4 *>(row + 4 * c) = make_float4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
}

__global__ void __launch_bounds__(64) k_attn17_f32(const float *__restrict__ qkv, float *__restrict__ o, int64_t B, int H, float scale) {
    __shared__ float Ks[PAIRS * PSTRIDE], Vs[PAIRS * PSTRIDE];
    const int lane = threadIdx.x, pl = lane / SK, i = lane - pl * SK;
    const int64_t pair = (int64_t)blockIdx.x * PAIRS + pl;
    const bool active = pl < PAIRS && pair < B * H;
    const int64_t b = active ? pair / H : 0;
    const int hd = active ? (int)(pair - b * H) : 0;
    const int D = HD * H;
    float q[HD], t[HD];
    if (active) {
        const float *tokp = qkv + (b * SK + i) * (int64_t)(3 * D) + hd * HD;
        load_row_f32(tokp + D, t);
        put_row_f32(Ks + pl * PSTRIDE + i * ROW, t);
        load_row_f32(tokp + 2 * D, t);
        put_row_f32(Vs + pl * PSTRIDE + i * ROW, t);
        load_row_f32(tokp, q);
    }
    __syncthreads();
    if (!active) return;
    // (the loops over the keys stay rolled, as in k_attn_fwd17: unrolled, the LDS reads of every row are hoisted into registers)
    float s[SK], m = -3.0e38f;
#pragma unroll 1
    for (int j = 0; j < SK; ++j) {
        const float *row = Ks + pl * PSTRIDE + j * ROW;
        float d = 0.f;
        for (int c = 0; c < HD / 4; ++c) {
            const float4 kv = *reinterpret_cast<const float4 *>(row + 4 * c);
            d = fmaf(q[4 * c], kv.x, d); d = fmaf(q[4 * c + 1], kv.y, d);
            d = fmaf(q[4 * c + 2], kv.z, d); d = fmaf(q[4 * c + 3], kv.w, d);
        }
        s[j] = d * scale;
        m = fmaxf(m, s[j]);
    }
    float l = 0.f;
    for (int j = 0; j < SK; ++j) {
        s[j] = expf(s[j] - m);
        l += s[j];
    }
    const float inv = 1.0f / l;
    float acc[HD];
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll 1
    for (int j = 0; j < SK; ++j) {
        const float pj = s[j] * inv;
        const float *row = Vs + pl * PSTRIDE + j * ROW;
        for (int c = 0; c < HD / 4; ++c) {
            const float4 kv = *reinterpret_cast<const float4 *>(row + 4 * c);
            acc[4 * c] = fmaf(pj, kv.x, acc[4 * c]); acc[4 * c + 1] = fmaf(pj, kv.y, acc[4 * c + 1]);
            acc[4 * c + 2] = fmaf(pj, kv.z, acc[4 * c + 2]); acc[4 * c + 3] = fmaf(pj, kv.w, acc[4 * c + 3]);
        }
    }
    put_row_f32(o + (b * SK + i) * (int64_t)D + hd * HD, acc);
}

// ------------------------------------------------------------------------------------------------ embedding + first LayerNorm
// One wavefront per token row (4 features per lane).  table f32 [16][31][256] = positional code + embedding row per (cell, tile).
__global__ void __launch_bounds__(256) k_embed_ln_f32(const uint8_t *__restrict__ boards, const float *__restrict__ table,
                                                      const float *__restrict__ cls, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, float eps, float *__restrict__ x0,
                                                      float *__restrict__ hn, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / 17;
    const int t = (int)(row - b * 17);
    const float *src = cls;
    if (t > 0) {
        int tile = boards[b * 16 + t - 1];
        tile = tile > 30 ? 30 : tile;
        src = table + ((size_t)(t - 1) * 31 + tile) * 256;
    }
    const float4 v = *reinterpret_cast<const float4 *>(src + 4 * lane);
    *reinterpret_cast<float4 *>(x0 + row * 256 + 4 * lane) = v;
    float sum = (v.x + v.y) + (v.z + v.w);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum * (1.0f / 256.0f);
    const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    float ss = fmaf(d0, d0, fmaf(d1, d1, fmaf(d2, d2, d3 * d3)));
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / 256.0f) + eps);
    const float4 ga = *reinterpret_cast<const float4 *>(gamma + 4 * lane), be = *reinterpret_cast<const float4 *>(beta + 4 * lane);
    *reinterpret_cast<float4 *>(hn + row * 256 + 4 * lane) =
        make_float4(d0 * rstd * ga.x + be.x, d1 * rstd * ga.y + be.y, d2 * rstd * ga.z + be.z, d3 * rstd * ga.w + be.w);
}

// a positive, finite power of two whose reciprocal is finite too
inline bool pow2(float s) {
    int e;
    return s > 0.f && isfinite(s) && frexpf(s, &e) == 0.5f && e > -120 && e < 120;
}
inline bool gemm_shape(int K, int N) { return (K == 256 || K == 1024) && (N == 256 || N == 768 || N == 1024); }

}  // namespace

extern "C" int g2048_f32split_pack(const float *w, int N, int K, float scale, void *packed, void *stream) {
    if (!w || !packed || !gemm_shape(K, N) || !pow2(scale) || !aligned16(w, packed)) return G2048_EINVAL;
    const int64_t n = (int64_t)N * (K / 8);
    hipLaunchKernelGGL(k_split_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, N, K, scale, (f16x8 *)packed);
    return launch_status();
}

extern "C" int g2048_f32split_gemm(const float *x, int64_t ldx, const void *w_packed, const float *bias, float *y, int64_t ldy,
                                   const float *resid, const float *gamma, const float *beta, float *h, int64_t T, int K, int N,
                                   int epilogue, float sx, float sw, float eps, void *stream) {
    if (!x || !w_packed || !bias || !y || T <= 0 || T > ((int64_t)1 << 30) || !gemm_shape(K, N) || !pow2(sx) || !pow2(sw)) return G2048_EINVAL;
    if (ldx < K || ldy < N || ((ldx | ldy) & 3) || !aligned16(x, w_packed, bias, y, resid, gamma, beta, h)) return G2048_EINVAL;
    const bool row = epilogue == G2048_F32SPLIT_ADD_LN || epilogue == G2048_F32SPLIT_ADD;
    if (row && (N != 256 || !resid)) return G2048_EINVAL;
    if (epilogue == G2048_F32SPLIT_ADD_LN && (!gamma || !beta || !h || !(eps > 0.f))) return G2048_EINVAL;
    const dim3 grid((unsigned)((T + 127) / 128), (unsigned)(N / 256)), block(256);
    const float inv = 1.0f / (sx * sw);
    if (!isfinite(inv) || inv == 0.f) return G2048_EINVAL;
    const f16x8 *wp = (const f16x8 *)w_packed;
    hipStream_t st = (hipStream_t)stream;
    switch (epilogue) {
    case G2048_F32SPLIT_BIAS:
        hipLaunchKernelGGL(k_split_gemm<G2048_F32SPLIT_BIAS>, grid, block, 0, st, x, ldx, wp, bias, y, ldy, resid, gamma, beta, h, T, K, sx, inv, eps);
        break;
    case G2048_F32SPLIT_BIAS_RELU:
        hipLaunchKernelGGL(k_split_gemm<G2048_F32SPLIT_BIAS_RELU>, grid, block, 0, st, x, ldx, wp, bias, y, ldy, resid, gamma, beta, h, T, K, sx, inv, eps);
        break;
    case G2048_F32SPLIT_ADD_LN:
        hipLaunchKernelGGL(k_split_gemm<G2048_F32SPLIT_ADD_LN>, grid, block, 0, st, x, ldx, wp, bias, y, ldy, resid, gamma, beta, h, T, K, sx, inv, eps);
        break;
    case G2048_F32SPLIT_ADD:
        hipLaunchKernelGGL(k_split_gemm<G2048_F32SPLIT_ADD>, grid, block, 0, st, x, ldx, wp, bias, y, ldy, resid, gamma, beta, h, T, K, sx, inv, eps);
        break;
    default:
        return G2048_EINVAL;
    }
    return launch_status();
}

extern "C" int g2048_attn_fwd_f32(const float *qkv, float *o, int64_t B, int H, float scale, void *stream) {
    if (!qkv || !o || B <= 0 || H <= 0 || H > 64 || B > ((int64_t)1 << 26) || !aligned16(qkv, o)) return G2048_EINVAL;
    const int64_t pairs = B * H;
    hipLaunchKernelGGL(k_attn17_f32, dim3((unsigned)((pairs + PAIRS - 1) / PAIRS)), dim3(64), 0, (hipStream_t)stream, qkv, o, B, H, scale);
    return launch_status();
}

extern "C" int g2048_embed_ln_f32(const uint8_t *boards, const float *table, const float *cls, const float *gamma, const float *beta,
                                  float eps, float *x0, float *h, int64_t B, void *stream) {
    if (!boards || !table || !cls || !gamma || !beta || !x0 || !h || B <= 0 || B > ((int64_t)1 << 26) || !(eps > 0.f) ||
        !aligned16(table, cls, gamma, beta, x0, h))
        return G2048_EINVAL;
    const int64_t rows = B * 17;
    hipLaunchKernelGGL(k_embed_ln_f32, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, boards, table, cls, gamma, beta, eps,
                       x0, h, rows);
    return launch_status();
}
