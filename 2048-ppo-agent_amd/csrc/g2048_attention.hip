// Attention forward/backward for the policy's tiny sequences (17 tokens, head_dim 32) in the PPO update.
//
// Replaces torch's scaled_dot_product_attention in training (reference: nn.TransformerEncoderLayer inside
// src/ppo/transformer_encoder.py:138-148, attention dropout 0.1).  The flash kernels PyTorch dispatches to spend
// 55 us forward and 217 us backward per layer at minibatch 2048 on problems of 17 x 17 scores per (sample, head);
// here one lane owns one query row (3 (sample, head) pairs per wavefront), K/V/Q/dO rows sit in LDS as f32, the
// 17 x 17 probabilities live in registers, and the whole thing is a few thousand VALU FMAs per lane: memory-bound.
// Dropout masks are recomputed in the backward pass from (seed, element index) instead of being stored.
//
// Layout: q/k/v/dq/dk/dv are bf16 with arbitrary (batch, token) strides and heads contiguous inside a token
// ([.., H, 32]), so they can point into the packed in_proj output / its gradient; o/dout are bf16 [B, Sq, H, 32]
// contiguous; lse f32 [B, H, Sq].  Sq = 17 (full layer) or 1 (CLS-only last layer), Sk = 17.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_mfma.h"

namespace {

using namespace g2048_mfma;
using namespace g2048_host;

constexpr int HD = 32, SK = 17, PAIRS = 3;  // (sample, head) pairs per wavefront when Sq = 17
constexpr int ROW = HD + 4;                  // f32 row stride in LDS (pad: pairs land on different banks)
constexpr int PSTRIDE = SK * ROW + 8;        // per-pair stride of a [17][32] f32 tile

struct Params {
    const uint16_t *q, *k, *v;
    int64_t B;
    int H;
    int64_t q_sb, q_ss, k_sb, k_ss, v_sb, v_ss;
    float scale, p_drop, inv_keep;
    uint32_t seed0, seed1, thr;
    const uint64_t *seed_state;  // optional device-resident word mixed into the seed (advanced between hipGraph replays)
};

// 32 bf16 (64 B) -> 32 f32
__device__ __forceinline__ void load_row(const uint16_t *p, float out[HD]) {
    const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
    for (int c = 0; c < 4; ++c) {
        const uint4 u = p4[c];
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
        for (int e = 0; e < 4; ++e) {
            out[8 * c + 2 * e] = __uint_as_float(w[e] << 16);
            out[8 * c + 2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u);
        }
    }
}
__device__ __forceinline__ void store_row(uint16_t *p, const float in[HD]) {
    uint4 *p4 = reinterpret_cast<uint4 *>(p);
    for (int c = 0; c < 4; ++c) {
        uint32_t w[4];
        for (int e = 0; e < 4; ++e) w[e] = pack2(in[8 * c + 2 * e], in[8 * c + 2 * e + 1]);
        p4[c] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// Workgroup -> work item, XCD-aware.  The dispatcher deals consecutive workgroup ids round-robin over the 8 XCDs, each with its
// own L2, while consecutive (sample, head) pairs share cache lines (the 64-byte q/k/v rows of neighbouring heads are halves
// of one 128-byte line, the 8 heads of a token one 512-byte run).  Give every XCD a contiguous range of items instead: XCD x
// gets the workgroups b with b % 8 == x, count_x = n / 8 + (x < n % 8) of them, and they take the items
// [start_x, start_x + count_x) with start_x = x * (n / 8) + min(x, n % 8) - a bijection of [0, n).
// (rocprofv3 FETCH_SIZE before: 1.35x the algorithmic reads.)
__device__ __forceinline__ int64_t xcd_block() {
    const int64_t n = gridDim.x, q = n / 8, r = n % 8, x = blockIdx.x % 8;
    return x * q + (x < r ? x : r) + blockIdx.x / 8;
}

// dropout keep decision for probability element `idx`: a 32-bit mix of (seed, idx), deterministic across fwd/bwd
__device__ __forceinline__ bool keep_mask(const Params &P, uint64_t idx) {
    return keep_elem(P.seed0, P.seed1, P.thr, idx);
}
// The same decision for element base + c when the caller has m = (uint32_t)base * HASH_MUL at hand: (base + c) * C = base * C + c * C
// (mod 2^32), so a run of elements costs one add of a compile-time constant each instead of a 64-bit add and two of the four
// quarter-rate v_mul_lo_u32.  SMALL (host-checked: every element index of the launch is below 2^32): the high word adds nothing
// but seed1.  Otherwise the plain form.
template <bool SMALL>
__device__ __forceinline__ bool keep_rel(const Params &P, uint64_t base, uint32_t m, uint32_t c) {
    if constexpr (!SMALL) return keep_mask(P, base + c);
    uint32_t x = (m + c * HASH_MUL) ^ (P.seed0 ^ P.seed1);
    G2048_HASH_FIN(x);
    return (x >> 8) >= P.thr;
}

__device__ __forceinline__ float dot_lds(const float a[HD], const float *row) {
    float s = 0.f;
    for (int c = 0; c < HD / 4; ++c) {
        const float4 kv = *reinterpret_cast<const float4 *>(row + 4 * c);
        s = fmaf(a[4 * c], kv.x, s); s = fmaf(a[4 * c + 1], kv.y, s);
        s = fmaf(a[4 * c + 2], kv.z, s); s = fmaf(a[4 * c + 3], kv.w, s);
    }
    return s;
}
__device__ __forceinline__ void axpy_lds(float acc[HD], float a, const float *row) {
    for (int c = 0; c < HD / 4; ++c) {
        const float4 kv = *reinterpret_cast<const float4 *>(row + 4 * c);
        acc[4 * c] = fmaf(a, kv.x, acc[4 * c]); acc[4 * c + 1] = fmaf(a, kv.y, acc[4 * c + 1]);
        acc[4 * c + 2] = fmaf(a, kv.z, acc[4 * c + 2]); acc[4 * c + 3] = fmaf(a, kv.w, acc[4 * c + 3]);
    }
}
__device__ __forceinline__ void put_row(float *row, const float v[HD]) {
    for (int c = 0; c < HD / 4; ++c) *reinterpret_cast<float4 *>(row + 4 * c) = make_float4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
}

// ------------------------------------------------------------------------------------------------ Sq = 17
__global__ void __launch_bounds__(64) k_attn_fwd17(Params P, uint16_t *__restrict__ o, float *__restrict__ lse) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    __shared__ float Ks[PAIRS * PSTRIDE], Vs[PAIRS * PSTRIDE];
    const int lane = threadIdx.x, pl = lane / SK, i = lane - pl * SK;
    const int64_t pair = xcd_block() * PAIRS + pl;
    const bool active = pl < PAIRS && pair < P.B * P.H;
    const int64_t b = active ? pair / P.H : 0;
    const int h = active ? (int)(pair - b * P.H) : 0;
    float q[HD], t[HD];
    if (active) {
        load_row(P.k + b * P.k_sb + i * P.k_ss + h * HD, t);
        put_row(Ks + pl * PSTRIDE + i * ROW, t);
        load_row(P.v + b * P.v_sb + i * P.v_ss + h * HD, t);
        put_row(Vs + pl * PSTRIDE + i * ROW, t);
        load_row(P.q + b * P.q_sb + i * P.q_ss + h * HD, q);
    }
    __syncthreads();
    if (!active) return;
    // The loops over the 17 keys stay ROLLED (s[] lives in registers through indexed moves): fully unrolled, the
    // compiler hoists the LDS reads of every row, needs all 512 registers plus scratch and runs one wave per SIMD.
    float s[SK], m = -3.0e38f;
#pragma unroll 1
    for (int j = 0; j < SK; ++j) {
        s[j] = dot_lds(q, Ks + pl * PSTRIDE + j * ROW) * P.scale;
        m = fmaxf(m, s[j]);
    }
    float l = 0.f;
    for (int j = 0; j < SK; ++j) {
        s[j] = __expf(s[j] - m);
        l += s[j];
    }
    const float inv = 1.0f / l;
    const uint64_t base = ((uint64_t)pair * SK + i) * 32;
    float acc[HD];
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll 1
    for (int j = 0; j < SK; ++j) {
        const float pj = (P.p_drop > 0.f && !keep_mask(P, base + j)) ? 0.f : s[j] * inv * P.inv_keep;
        axpy_lds(acc, pj, Vs + pl * PSTRIDE + j * ROW);
    }
    store_row(o + ((b * SK + i) * P.H + h) * HD, acc);
    lse[(b * P.H + h) * SK + i] = m + __logf(l);
}

__global__ void __launch_bounds__(64) k_attn_bwd17(Params P, const uint16_t *__restrict__ dout, const float *__restrict__ lse,
                                                   uint16_t *__restrict__ dq, uint16_t *__restrict__ dk,
                                                   uint16_t *__restrict__ dv) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    // K/V tiles serve the first phase (dS, dQ), then the same LDS holds Q/dO for the second (dK, dV): 22 KB per
    // workgroup instead of 37, i.e. 7 resident waves per CU instead of 4
    __shared__ float Ks[PAIRS * PSTRIDE], Vs[PAIRS * PSTRIDE];
    __shared__ float dSs[PAIRS * SK * (SK + 1)], Pt[PAIRS * SK * (SK + 1)];
    float *const Qs = Ks, *const Gs = Vs;
    const int lane = threadIdx.x, pl = lane / SK, i = lane - pl * SK;
    const int64_t pair = xcd_block() * PAIRS + pl;
    const bool active = pl < PAIRS && pair < P.B * P.H;
    const int64_t b = active ? pair / P.H : 0;
    const int h = active ? (int)(pair - b * P.H) : 0;
    float q[HD], g[HD], t[HD];
    if (active) {
        load_row(P.k + b * P.k_sb + i * P.k_ss + h * HD, t);
        put_row(Ks + pl * PSTRIDE + i * ROW, t);
        load_row(P.v + b * P.v_sb + i * P.v_ss + h * HD, t);
        put_row(Vs + pl * PSTRIDE + i * ROW, t);
        load_row(P.q + b * P.q_sb + i * P.q_ss + h * HD, q);
        load_row(dout + ((b * SK + i) * P.H + h) * HD, g);
    }
    __syncthreads();
    if (active) {
        const float L = lse[(b * P.H + h) * SK + i];
        const uint64_t base = ((uint64_t)pair * SK + i) * 32;
        float p[SK], dp[SK], delta = 0.f;
#pragma unroll 1
        for (int j = 0; j < SK; ++j) {
            p[j] = __expf(dot_lds(q, Ks + pl * PSTRIDE + j * ROW) * P.scale - L);
            const bool keep = !(P.p_drop > 0.f) || keep_mask(P, base + j);
            dp[j] = keep ? dot_lds(g, Vs + pl * PSTRIDE + j * ROW) * P.inv_keep : 0.f;
            delta = fmaf(p[j], dp[j], delta);
            Pt[(pl * SK + i) * (SK + 1) + j] = keep ? p[j] * P.inv_keep : 0.f;
        }
        float acc[HD];
        for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll 1
        for (int j = 0; j < SK; ++j) {
            const float ds = p[j] * (dp[j] - delta) * P.scale;
            dSs[(pl * SK + i) * (SK + 1) + j] = ds;
            axpy_lds(acc, ds, Ks + pl * PSTRIDE + j * ROW);
        }
        store_row(dq + b * P.q_sb + i * P.q_ss + h * HD, acc);
    }
    __syncthreads();  // every lane is done with K/V
    if (active) {
        put_row(Qs + pl * PSTRIDE + i * ROW, q);
        put_row(Gs + pl * PSTRIDE + i * ROW, g);
    }
    __syncthreads();
    if (!active) return;
    // this lane now owns key/value row j = i of its pair
    float ak[HD], av[HD];
    for (int d = 0; d < HD; ++d) ak[d] = av[d] = 0.f;
#pragma unroll 1
    for (int r = 0; r < SK; ++r) {
        axpy_lds(ak, dSs[(pl * SK + r) * (SK + 1) + i], Qs + pl * PSTRIDE + r * ROW);
        axpy_lds(av, Pt[(pl * SK + r) * (SK + 1) + i], Gs + pl * PSTRIDE + r * ROW);
    }
    store_row(dk + b * P.k_sb + i * P.k_ss + h * HD, ak);
    store_row(dv + b * P.v_sb + i * P.v_ss + h * HD, av);
}

// ------------------------------------------------------------------------------------------------ Sq = 1 (CLS row)
__global__ void __launch_bounds__(64) k_attn_fwd1(Params P, uint16_t *__restrict__ o, float *__restrict__ lse) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    const int64_t pair = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (pair >= P.B * P.H) return;
    const int64_t b = pair / P.H;
    const int h = (int)(pair - b * P.H);
    float q[HD], t[HD], s[SK], m = -3.0e38f;
    load_row(P.q + b * P.q_sb + h * HD, q);
    for (int j = 0; j < SK; ++j) {
        load_row(P.k + b * P.k_sb + j * P.k_ss + h * HD, t);
        float a = 0.f;
        for (int d = 0; d < HD; ++d) a = fmaf(q[d], t[d], a);
        s[j] = a * P.scale;
        m = fmaxf(m, s[j]);
    }
    float l = 0.f;
    for (int j = 0; j < SK; ++j) {
        s[j] = __expf(s[j] - m);
        l += s[j];
    }
    const float inv = 1.0f / l;
    float acc[HD];
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
    for (int j = 0; j < SK; ++j) {
        const float pj = (P.p_drop > 0.f && !keep_mask(P, (uint64_t)pair * 32 + j)) ? 0.f : s[j] * inv * P.inv_keep;
        load_row(P.v + b * P.v_sb + j * P.v_ss + h * HD, t);
        for (int d = 0; d < HD; ++d) acc[d] = fmaf(pj, t[d], acc[d]);
    }
    store_row(o + (b * P.H + h) * HD, acc);
    lse[b * P.H + h] = m + __logf(l);
}

__global__ void __launch_bounds__(64) k_attn_bwd1(Params P, const uint16_t *__restrict__ dout, const float *__restrict__ lse,
                                                  uint16_t *__restrict__ dq, uint16_t *__restrict__ dk,
                                                  uint16_t *__restrict__ dv) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    const int64_t pair = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (pair >= P.B * P.H) return;
    const int64_t b = pair / P.H;
    const int h = (int)(pair - b * P.H);
    float q[HD], g[HD], t[HD], p[SK], dp[SK], delta = 0.f;
    load_row(P.q + b * P.q_sb + h * HD, q);
    load_row(dout + (b * P.H + h) * HD, g);
    const float L = lse[b * P.H + h];
    for (int j = 0; j < SK; ++j) {
        load_row(P.k + b * P.k_sb + j * P.k_ss + h * HD, t);
        float a = 0.f;
        for (int d = 0; d < HD; ++d) a = fmaf(q[d], t[d], a);
        p[j] = __expf(a * P.scale - L);
        const bool keep = !(P.p_drop > 0.f) || keep_mask(P, (uint64_t)pair * 32 + j);
        load_row(P.v + b * P.v_sb + j * P.v_ss + h * HD, t);
        float c = 0.f;
        for (int d = 0; d < HD; ++d) c = fmaf(g[d], t[d], c);
        dp[j] = keep ? c * P.inv_keep : 0.f;
        delta = fmaf(p[j], dp[j], delta);
        // dV_j = Ptilde_j * dO
        const float pt = keep ? p[j] * P.inv_keep : 0.f;
        for (int d = 0; d < HD; ++d) t[d] = pt * g[d];
        store_row(dv + b * P.v_sb + j * P.v_ss + h * HD, t);
    }
    float acc[HD];
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
    for (int j = 0; j < SK; ++j) {
        const float ds = p[j] * (dp[j] - delta) * P.scale;
        load_row(P.k + b * P.k_sb + j * P.k_ss + h * HD, t);
        for (int d = 0; d < HD; ++d) acc[d] = fmaf(ds, t[d], acc[d]);
        for (int d = 0; d < HD; ++d) t[d] = ds * q[d];
        store_row(dk + b * P.k_sb + j * P.k_ss + h * HD, t);
    }
    store_row(dq + b * P.q_sb + h * HD, acc);
}

// ------------------------------------------------------------------------------------------------ Sq = 1, row-coalesced
// k_attn_fwd1 / k_attn_bwd1 give a lane a whole (sample, head) pair: 2048 x 8 pairs are 256 wavefronts, one per CU, each walking
// 17 + 17 dependent 64-byte rows (19 / 31 us for 36 MB of K/V: 1.9 TB/s).  For H = 8 the eight heads of a token are one 512-byte
// run of the packed K/V projection: here a 32-lane group owns a SAMPLE, lane (h, c) the 16-byte chunk c of head h, so every
// K_j / V_j fetch of a group is one contiguous 512-byte row and there are 4x the wavefronts.  A head's score is a 4-lane sum
// (2 shuffles), the softmax over the 17 keys and both sums over keys (O, dQ) are in-lane, dK_j / dV_j are stored as the same
// 512-byte rows.  (First attempt, one lane per KEY with a transposing 31-shuffle reduction: rows of 17 different tokens per load
// instruction - 55 / 63 us, three times slower than the scalar kernels.)  Dropout uses the scalar kernels' element index.
__device__ __forceinline__ void unpack8(const uint4 u, float f[8]) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = __uint_as_float(w[e] << 16);
        f[2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u);
    }
}
__device__ __forceinline__ uint4 pack8(const float f[8]) {
    return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
}
__device__ __forceinline__ float quad_dot(const float a[8], const uint4 u) {
    float f[8], s = 0.f;
    unpack8(u, f);
    for (int d = 0; d < 8; ++d) s = fmaf(a[d], f[d], s);
    s += __shfl_xor(s, 1);
    return s + __shfl_xor(s, 2);
}

__global__ void __launch_bounds__(256) k_attn_fwd1_rows(Params P, uint16_t *__restrict__ o, float *__restrict__ lse) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    const int l = threadIdx.x & 31, h = l >> 2, c = l & 3;
    const int64_t b = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (b >= P.B) return;  // (a whole 32-lane group)
    const int64_t pair = b * 8 + h;
    const int col = h * HD + 8 * c;
    float q[8], s[SK], acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unpack8(*reinterpret_cast<const uint4 *>(P.q + b * P.q_sb + col), q);
    uint4 kk[SK], vv[SK];
#pragma unroll
    for (int j = 0; j < SK; ++j) kk[j] = *reinterpret_cast<const uint4 *>(P.k + b * P.k_sb + j * P.k_ss + col);
#pragma unroll
    for (int j = 0; j < SK; ++j) vv[j] = *reinterpret_cast<const uint4 *>(P.v + b * P.v_sb + j * P.v_ss + col);
    float m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
        s[j] = quad_dot(q, kk[j]) * P.scale;
        m = fmaxf(m, s[j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
        s[j] = __expf(s[j] - m);
        sum += s[j];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
        const float pj = (P.p_drop > 0.f && !keep_mask(P, (uint64_t)pair * 32 + j)) ? 0.f : s[j] * inv * P.inv_keep;
        float v[8];
        unpack8(vv[j], v);
        for (int d = 0; d < 8; ++d) acc[d] = fmaf(pj, v[d], acc[d]);
    }
    *reinterpret_cast<uint4 *>(o + b * (8 * HD) + col) = pack8(acc);
    if (c == 0) lse[pair] = m + __logf(sum);
}

__global__ void __launch_bounds__(256) k_attn_bwd1_rows(Params P, const uint16_t *__restrict__ dout, const float *__restrict__ lse,
                                                        uint16_t *__restrict__ dq, uint16_t *__restrict__ dk,
                                                        uint16_t *__restrict__ dv) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    const int l = threadIdx.x & 31, h = l >> 2, c = l & 3;
    const int64_t b = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (b >= P.B) return;
    const int64_t pair = b * 8 + h;
    const int col = h * HD + 8 * c;
    float q[8], g[8], p[SK], dp[SK], acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unpack8(*reinterpret_cast<const uint4 *>(P.q + b * P.q_sb + col), q);
    unpack8(*reinterpret_cast<const uint4 *>(dout + b * (8 * HD) + col), g);
    uint4 kk[SK], vv[SK];
#pragma unroll
    for (int j = 0; j < SK; ++j) kk[j] = *reinterpret_cast<const uint4 *>(P.k + b * P.k_sb + j * P.k_ss + col);
#pragma unroll
    for (int j = 0; j < SK; ++j) vv[j] = *reinterpret_cast<const uint4 *>(P.v + b * P.v_sb + j * P.v_ss + col);
    const float L = lse[pair];
    float delta = 0.f;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
        p[j] = __expf(quad_dot(q, kk[j]) * P.scale - L);
        const bool keep = !(P.p_drop > 0.f) || keep_mask(P, (uint64_t)pair * 32 + j);
        dp[j] = keep ? quad_dot(g, vv[j]) * P.inv_keep : 0.f;
        delta = fmaf(p[j], dp[j], delta);
        const float pt = keep ? p[j] * P.inv_keep : 0.f;  // dV_j = Ptilde_j * dO
        float t[8];
        for (int d = 0; d < 8; ++d) t[d] = pt * g[d];
        *reinterpret_cast<uint4 *>(dv + b * P.v_sb + j * P.v_ss + col) = pack8(t);
    }
#pragma unroll
    for (int j = 0; j < SK; ++j) {
        const float ds = p[j] * (dp[j] - delta) * P.scale;  // dK_j = ds_j * q,  dQ = sum_j ds_j * K_j
        float t[8], kf[8];
        unpack8(kk[j], kf);
        for (int d = 0; d < 8; ++d) {
            acc[d] = fmaf(ds, kf[d], acc[d]);
            t[d] = ds * q[d];
        }
        *reinterpret_cast<uint4 *>(dk + b * P.k_sb + j * P.k_ss + col) = pack8(t);
    }
    *reinterpret_cast<uint4 *>(dq + b * P.q_sb + col) = pack8(acc);
}

// ------------------------------------------------------------------------------------------------ Sq = 17 on MFMA
// The 17 x 17 problems of one (sample, head) pair mapped onto v_mfma_f32_32x32x16_bf16 tiles (17 of 32 rows and columns
// used: the matrix cores are idle either way, the point is to take the ~2700 f32 FMAs per lane off the vector ALU and the
// K/V rows out of LDS).  One wavefront owns one sample and walks its heads; everything is computed TRANSPOSED so that a
// lane owns one QUERY column of every tile and the softmax statistics are per lane:
//   S^T[key][q] = K . Q^T        A = K rows (lane = key, 8 consecutive d), B = Q rows (lane = query, 8 consecutive d): both
//                                 operands are plain 16-byte global loads, no LDS
//   P^T         = softmax over the 16 accumulator registers of a lane + the other half-wave (lane ^ 32)
//   O^T[d][q]   = V^T . P^T      B = P^T straight from the accumulator registers (register i of half h is key
//                                 (i & 3) + 8 (i >> 2) + 4 h: the A operand V^T is gathered from an LDS copy of V in the
//                                 same key order, 9 two-byte reads per lane); the result has 8 consecutive d per lane
//                                 after one v_permlane32_swap -> 16-byte stores
// Dropout uses the element index of the scalar kernels ((pair * 17 + q) * 32 + key), so forward and backward of either
// implementation can be mixed.
// LDS hand-over inside ONE wavefront (these kernels run 64-thread workgroups): the LDS unit executes a wave's DS instructions in
// order, so all that is needed is that earlier DS traffic has been issued and returned before the dependent reads - not the
// vmcnt(0) + s_barrier of __syncthreads(), which would also drain the global prefetch of the next head
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ float xhalf(float x) { return __shfl_xor(x, 32); }

template <bool SMALL>
__global__ void __launch_bounds__(64) k_attn_fwd17_mfma(Params P, uint16_t *__restrict__ o, float *__restrict__ lse) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    __shared__ __attribute__((aligned(16))) uint16_t Vs[SK * HD];  // V of the current head, [17][32] bf16
    const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
    // grid = B * splits: a wavefront owns heads [h0, h1) of one sample (splits = 2 doubles the waves in flight per CU)
    const int splits = (int)(gridDim.x / P.B);
    const int64_t item = xcd_block(), b = item / splits;
    const int hpw = (P.H + splits - 1) / splits, h0 = (int)(item - b * splits) * hpw, h1 = h0 + hpw < P.H ? h0 + hpw : P.H;
    const bool row_ok = r < SK;
    const int rr = row_ok ? r : 0;
    const float c_log2 = P.scale * 1.4426950408889634f;
    const bool no_drop = !(P.p_drop > 0.f);
    const uint32_t lane_km = (uint32_t)(r * 32 + 4 * hf) * HASH_MUL;  // the lane's share of keep_rel's m
    const uint16_t *kb = P.k + b * P.k_sb + rr * P.k_ss + 8 * hf, *qb = P.q + b * P.q_sb + rr * P.q_ss + 8 * hf;
    const uint16_t *vb = P.v + b * P.v_sb + (lane >> 2) * P.v_ss + 8 * (lane & 3);  // rows 0..15: one 16-byte chunk per lane
    const uint16_t *v16 = P.v + b * P.v_sb + 16 * P.v_ss + 8 * (lane & 3);          // row 16: lanes 0..3
    struct Op { uint4 k0, k1, q0, q1, vr, vl; };  // the operands of one head, by value (registers)
    const uint32_t live = row_ok ? 0xFFFFFFFFu : 0u;
    auto zpad = [&](uint4 u) { return make_uint4(u.x & live, u.y & live, u.z & live, u.w & live); };
    auto fetch = [&](int h) -> Op {
        Op x;
        // unconditional loads (padding lanes read row 0 through the clamped address and are zeroed by zpad below): a load
        // under a divergent branch gets a vmcnt(0) at the join, which serialises the prefetch
        x.k0 = *reinterpret_cast<const uint4 *>(kb + h * HD);
        x.k1 = *reinterpret_cast<const uint4 *>(kb + h * HD + 16);
        x.q0 = *reinterpret_cast<const uint4 *>(qb + h * HD);
        x.q1 = *reinterpret_cast<const uint4 *>(qb + h * HD + 16);
        x.vr = *reinterpret_cast<const uint4 *>(vb + h * HD);
        x.vl = *reinterpret_cast<const uint4 *>(v16 + h * HD);
        return x;
    };
    Op nx;
    if (h0 < h1) nx = fetch(h0);
    for (int h = h0; h < h1; ++h) {
        const int64_t pair = b * P.H + h;
        Op c = nx;
        c.k0 = zpad(c.k0); c.k1 = zpad(c.k1); c.q0 = zpad(c.q0); c.q1 = zpad(c.q1);
        // ---- S^T = K Q^T
        f32x16 st;
        _Pragma("unroll") for (int i = 0; i < 16; ++i) st[i] = 0.f;
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, c.k0), __builtin_bit_cast(bf16x8, c.q0), st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, c.k1), __builtin_bit_cast(bf16x8, c.q1), st, 0, 0, 0);
        // ---- V of this head -> LDS (the previous head's reads are done: same wave, LDS is in order; barrier for the compiler)
        wave_lds_sync();
        *reinterpret_cast<uint4 *>(Vs + (lane >> 2) * HD + 8 * (lane & 3)) = c.vr;
        if (lane < 4) *reinterpret_cast<uint4 *>(Vs + 16 * HD + 8 * lane) = c.vl;
        wave_lds_sync();
        if (h + 1 < h1) nx = fetch(h + 1);  // next head's operands in flight behind the softmax
        // ---- softmax over the keys of this lane's query (registers 0..7 are keys < 16, register 8 of half 0 is key 16)
        float m = -3.0e38f;
        _Pragma("unroll") for (int i = 0; i < 8; ++i) m = fmaxf(m, st[i]);
        if (hf == 0) m = fmaxf(m, st[8]);
        m = fmaxf(m, xhalf(m));
        float p[9], l = 0.f;
        _Pragma("unroll") for (int i = 0; i < 8; ++i) {
            p[i] = exp2f((st[i] - m) * c_log2);
            l += p[i];
        }
        p[8] = hf == 0 ? exp2f((st[8] - m) * c_log2) : 0.f;
        l += p[8];
        l += xhalf(l);
        const float inv = P.inv_keep / l;
        const uint64_t base = ((uint64_t)pair * SK + r) * 32 + 4 * hf;  // rowof(i, hf) = (i & 3) + 8 (i >> 2) + 4 hf
        const uint32_t km = (uint32_t)(pair * (SK * 32)) * HASH_MUL + lane_km;
        _Pragma("unroll") for (int i = 0; i < 9; ++i) {
            const bool keep = no_drop | keep_rel<SMALL>(P, base, km, rowof(i, 0));  // (bitwise: no branch per element)
            p[i] = keep ? p[i] * inv : 0.f;
        }
        const uint4 pb0 = make_uint4(pack2(p[0], p[1]), pack2(p[2], p[3]), pack2(p[4], p[5]), pack2(p[6], p[7]));
        const uint4 pb1 = make_uint4(pack2(p[8], 0.f), 0u, 0u, 0u);
        // ---- V^T in the accumulator's key order: lane = feature d
        uint32_t w[4];
        _Pragma("unroll") for (int j = 0; j < 8; j += 2)
            w[j >> 1] = (uint32_t)Vs[rowof(j, hf) * HD + r] | ((uint32_t)Vs[rowof(j + 1, hf) * HD + r] << 16);
        const uint4 va0 = make_uint4(w[0], w[1], w[2], w[3]);
        const uint4 va1 = make_uint4(hf == 0 ? (uint32_t)Vs[16 * HD + r] : 0u, 0u, 0u, 0u);
        // ---- O^T = V^T P^T
        f32x16 ot;
        _Pragma("unroll") for (int i = 0; i < 16; ++i) ot[i] = 0.f;
        ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va0), __builtin_bit_cast(bf16x8, pb0), ot, 0, 0, 0);
        ot = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va1), __builtin_bit_cast(bf16x8, pb1), ot, 0, 0, 0);
        // ---- lane (q, hf) holds d = rowof(i, hf): swap halves so that every lane owns 8 consecutive d, store
        uint16_t *orow = o + ((b * SK + rr) * P.H + h) * HD + 8 * hf;
        _Pragma("unroll") for (int mm = 0; mm < 2; ++mm) {
            uint32_t ax = pack2(ot[8 * mm + 0], ot[8 * mm + 1]), ay = pack2(ot[8 * mm + 2], ot[8 * mm + 3]);
            uint32_t bx = pack2(ot[8 * mm + 4], ot[8 * mm + 5]), by = pack2(ot[8 * mm + 6], ot[8 * mm + 7]);
            const auto sx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
            if (row_ok) *reinterpret_cast<uint4 *>(orow + 16 * mm) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
        }
        if (row_ok && hf == 0) lse[pair * SK + r] = m * P.scale + __logf(l);
    }
}

// Backward on MFMA tiles.  Two orientations of the same 17 x 17 problem, because every product wants its reduction index
// on the operands' "k" axis and its result rows on accumulator registers:
//   lane = QUERY column:  S^T = K Q^T, dP^T = V dO^T  ->  p, dropout, delta_q = sum_key p dp (per lane), dS^T
//                         dQ^T[d][q] = K^T dS^T        (B = dS^T from the accumulator registers, A = K^T gathered from LDS)
//   lane = KEY column:    S = Q K^T,  dP = dO V^T      ->  p, dropout again (lse_q and delta_q per REGISTER, from LDS), dS, P
//                         dK^T[d][key] = Q^T dS,  dV^T[d][key] = dO^T P_dropped
// The operand registers of Q, K, V, dO (lane = row, 8 consecutive d per half) serve as A in one orientation and as B in the
// other; their LDS copies ([17][32] bf16 each) only feed the three transposed gathers (9 two-byte reads per lane each).
// 14 MFMAs per (sample, head) instead of ~2700 FMAs per lane.
// One (sample, head) pair per wavefront, five of them resident per SIMD (82 registers; round 3): inside the update the kernel waits for HBM (its operands
// were written a whole forward pass ago), so what pays is pairs in flight, not a register-hungry prefetch of the next head inside
// a wave that walks several (rounds 1-2: 4 heads per wave, 146 + 32 registers = two waves per SIMD: 46.4 us per launch in the
// update's graph, 41.2 with one head per wave).
template <bool SMALL>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5)))
k_attn_bwd17_mfma(Params P, const uint16_t *__restrict__ dout, const float *__restrict__ lse,
                                                        uint16_t *__restrict__ dq, uint16_t *__restrict__ dk,
                                                        uint16_t *__restrict__ dv) {
    mix_seed_state(P.seed_state, P.seed0, P.seed1);
    __shared__ __attribute__((aligned(16))) uint16_t Ks[SK * HD], Qs[SK * HD], Gs[SK * HD];
    __shared__ float lseS[32], delS[32];
    const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
    const int64_t pair = xcd_block(), b = pair / P.H;  // grid = B * H
    const int h = (int)(pair - b * P.H);
    const bool row_ok = r < SK;
    const int rr = row_ok ? r : 0;
    const float c_log2 = P.scale * 1.4426950408889634f;
    const uint16_t *kb = P.k + b * P.k_sb + rr * P.k_ss + 8 * hf, *qb = P.q + b * P.q_sb + rr * P.q_ss + 8 * hf;
    const uint16_t *vb = P.v + b * P.v_sb + rr * P.v_ss + 8 * hf;
    const uint16_t *gb = dout + (b * SK + rr) * P.H * HD + 8 * hf;
    struct Op { uint4 k0, k1, q0, q1, v0, v1, g0, g1; float lq; };  // the operands of one head, by value (registers)
    const uint32_t live = row_ok ? 0xFFFFFFFFu : 0u;
    auto zpad = [&](uint4 u) { return make_uint4(u.x & live, u.y & live, u.z & live, u.w & live); };
    const bool no_drop = !(P.p_drop > 0.f);
    // the lane's share of keep_rel's m: lane = query (elements (pair * 17 + r) * 32 + key) and lane = key (... + query) * 32 + r)
    const uint32_t lane_km1 = (uint32_t)(r * 32 + 4 * hf) * HASH_MUL, lane_km2 = (uint32_t)(r + 128 * hf) * HASH_MUL;
    auto fetch = [&](int h) -> Op {
        Op x;
        const uint16_t *kp = kb + h * HD, *qp = qb + h * HD, *vp = vb + h * HD, *gp = gb + h * HD;
        // unconditional loads through clamped addresses, padding lanes zeroed afterwards (see the forward kernel)
        x.k0 = *reinterpret_cast<const uint4 *>(kp); x.k1 = *reinterpret_cast<const uint4 *>(kp + 16);
        x.q0 = *reinterpret_cast<const uint4 *>(qp); x.q1 = *reinterpret_cast<const uint4 *>(qp + 16);
        x.v0 = *reinterpret_cast<const uint4 *>(vp); x.v1 = *reinterpret_cast<const uint4 *>(vp + 16);
        x.g0 = *reinterpret_cast<const uint4 *>(gp); x.g1 = *reinterpret_cast<const uint4 *>(gp + 16);
        x.lq = lse[(b * P.H + h) * SK + rr];
        return x;
    };
    struct Frag { uint4 a, b; };
    auto mfma2 = [&](uint4 a0, uint4 a1, uint4 b0, uint4 b1) {
        f32x16 acc;
        _Pragma("unroll") for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), __builtin_bit_cast(bf16x8, b0), acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), __builtin_bit_cast(bf16x8, b1), acc, 0, 0, 0);
    };
    // registers 0..7 of a lane are rows rowof(i, hf) < 16, register 8 of half 0 is row 16; all others are padding
    auto gather = [&](const uint16_t *tile) -> Frag {  // tile^T in register order: lane = feature d
        uint32_t w[4];
        _Pragma("unroll") for (int j = 0; j < 8; j += 2) w[j >> 1] = (uint32_t)tile[rowof(j, hf) * HD + r] | ((uint32_t)tile[rowof(j + 1, hf) * HD + r] << 16);
        return Frag{make_uint4(w[0], w[1], w[2], w[3]), make_uint4(hf == 0 ? (uint32_t)tile[16 * HD + r] : 0u, 0u, 0u, 0u)};
    };
    auto store_rows = [&](const f32x16 &t, uint16_t *row) {  // lane (row r, hf) of a transposed result: d = rowof(i, hf)
        _Pragma("unroll") for (int mm = 0; mm < 2; ++mm) {
            uint32_t ax = pack2(t[8 * mm + 0], t[8 * mm + 1]), ay = pack2(t[8 * mm + 2], t[8 * mm + 3]);
            uint32_t bx = pack2(t[8 * mm + 4], t[8 * mm + 5]), by = pack2(t[8 * mm + 6], t[8 * mm + 7]);
            const auto sx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
            if (row_ok) *reinterpret_cast<uint4 *>(row + 16 * mm) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
        }
    };
#define G2048_AS_OPERAND(x) Frag{make_uint4(pack2(x[0], x[1]), pack2(x[2], x[3]), pack2(x[4], x[5]), pack2(x[6], x[7])), \
                                 make_uint4(pack2(x[8], 0.f), 0u, 0u, 0u)}
    {
        Op c = fetch(h);
        c.k0 = zpad(c.k0); c.k1 = zpad(c.k1); c.q0 = zpad(c.q0); c.q1 = zpad(c.q1);
        c.v0 = zpad(c.v0); c.v1 = zpad(c.v1); c.g0 = zpad(c.g0); c.g1 = zpad(c.g1);
        // ---- LDS copies of K, Q, dO (row-major) for the transposed gathers; lse per query
        if (row_ok) {
            *reinterpret_cast<uint4 *>(Ks + r * HD + 8 * hf) = c.k0; *reinterpret_cast<uint4 *>(Ks + r * HD + 16 + 8 * hf) = c.k1;
            *reinterpret_cast<uint4 *>(Qs + r * HD + 8 * hf) = c.q0; *reinterpret_cast<uint4 *>(Qs + r * HD + 16 + 8 * hf) = c.q1;
            *reinterpret_cast<uint4 *>(Gs + r * HD + 8 * hf) = c.g0; *reinterpret_cast<uint4 *>(Gs + r * HD + 16 + 8 * hf) = c.g1;
            if (hf == 0) lseS[r] = c.lq;
        }
        const float lq2 = c.lq * 1.4426950408889634f;
        // ---- orientation 1: lane = query
        const f32x16 st = mfma2(c.k0, c.k1, c.q0, c.q1), dpt = mfma2(c.v0, c.v1, c.g0, c.g1);
        float ds[9], delta = 0.f;
        {
            const uint64_t base = ((uint64_t)pair * SK + r) * 32 + 4 * hf;
            const uint32_t km = (uint32_t)(pair * (SK * 32)) * HASH_MUL + lane_km1;
            float p[9], dp[9];
            _Pragma("unroll") for (int i = 0; i < 9; ++i) {
                const bool valid = i < 8 || hf == 0;
                const bool keep = no_drop | keep_rel<SMALL>(P, base, km, rowof(i, 0));
                p[i] = valid ? exp2f(st[i] * c_log2 - lq2) : 0.f;
                dp[i] = (valid && keep) ? dpt[i] * P.inv_keep : 0.f;
                delta = fmaf(p[i], dp[i], delta);
            }
            delta += xhalf(delta);
            _Pragma("unroll") for (int i = 0; i < 9; ++i) ds[i] = p[i] * (dp[i] - delta) * P.scale;
        }
        if (row_ok && hf == 0) delS[r] = delta;
        wave_lds_sync();  // K/Q/dO tiles, lse and delta are in LDS
        const Frag dsb = G2048_AS_OPERAND(ds), kt = gather(Ks);
        store_rows(mfma2(kt.a, kt.b, dsb.a, dsb.b), dq + b * P.q_sb + rr * P.q_ss + h * HD + 8 * hf);
        // ---- orientation 2: lane = key, register i = query rowof(i, hf)
        const f32x16 s2 = mfma2(c.q0, c.q1, c.k0, c.k1), dp2 = mfma2(c.g0, c.g1, c.v0, c.v1);
        float ds2[9], pd2[9];
        const uint64_t base2 = (uint64_t)pair * (SK * 32) + r + 128 * hf;  // query rowof(i, hf): 32 x ((i & 3) + 8 (i >> 2)) more
        const uint32_t km2 = (uint32_t)(pair * (SK * 32)) * HASH_MUL + lane_km2;
        _Pragma("unroll") for (int i = 0; i < 9; ++i) {
            const bool valid = i < 8 || hf == 0;
            const int qi = valid ? rowof(i, hf) : 0;
            const bool keep = no_drop | keep_rel<SMALL>(P, base2, km2, 32 * rowof(i, 0));
            const float p = valid ? exp2f(s2[i] * c_log2 - lseS[qi] * 1.4426950408889634f) : 0.f;
            const float dp = (valid && keep) ? dp2[i] * P.inv_keep : 0.f;
            ds2[i] = p * (dp - delS[qi]) * P.scale;
            pd2[i] = keep ? p * P.inv_keep : 0.f;
        }
        const Frag ds2b = G2048_AS_OPERAND(ds2), pd2b = G2048_AS_OPERAND(pd2), qt = gather(Qs), gt = gather(Gs);
        store_rows(mfma2(qt.a, qt.b, ds2b.a, ds2b.b), dk + b * P.k_sb + rr * P.k_ss + h * HD + 8 * hf);
        store_rows(mfma2(gt.a, gt.b, pd2b.a, pd2b.b), dv + b * P.v_sb + rr * P.v_ss + h * HD + 8 * hf);
    }
#undef G2048_AS_OPERAND
}

inline bool fill(Params &P, const void *q, const void *k, const void *v, int64_t B, int H, int Sq, int64_t q_sb,
                 int64_t q_ss, int64_t k_sb, int64_t k_ss, int64_t v_sb, int64_t v_ss, float scale, float p_drop,
                 uint64_t seed, const uint64_t *seed_state) {
    if (!q || !k || !v || B <= 0 || H <= 0 || (Sq != 1 && Sq != SK) || !(p_drop >= 0.f && p_drop < 1.f)) return false;
    // rows are read/written as 4 x 16 bytes
    if (!aligned16(q, k, v)) return false;
    if ((q_sb | q_ss | k_sb | k_ss | v_sb | v_ss) & 7) return false;
    P.q = (const uint16_t *)q; P.k = (const uint16_t *)k; P.v = (const uint16_t *)v;
    P.B = B; P.H = H;
    P.q_sb = q_sb; P.q_ss = q_ss; P.k_sb = k_sb; P.k_ss = k_ss; P.v_sb = v_sb; P.v_ss = v_ss;
    P.scale = scale; P.p_drop = p_drop; P.inv_keep = 1.0f / (1.0f - p_drop);
    P.seed0 = (uint32_t)seed; P.seed1 = (uint32_t)(seed >> 32); P.seed_state = seed_state;
    P.thr = (uint32_t)(p_drop * 16777216.0f);
    return true;
}
// G2048_ATTN_SCALAR=1 keeps the scalar kernels (17-token: one lane per query row; CLS row: one lane per pair) (read per call: no
// latch, no library state)
// every dropout element index (pair * 17 + query) * 32 + key of the launch, padding lanes included, stays below 2^32
// (G2048_ATTN_WIDE_INDEX=1 forces the 64-bit form, which no realistic batch reaches: the tests compare the two bit for bit)
inline bool small_indices(int64_t pairs) {
    const char *e = getenv("G2048_ATTN_WIDE_INDEX");
    return pairs <= (int64_t)((1ull << 32) / (SK * 32)) - 2 && !(e && e[0] == '1');
}
inline bool use_mfma17() {
    const char *e = getenv("G2048_ATTN_SCALAR");
    return !(e && e[0] == '1');
}

}  // namespace

extern "C" int g2048_attn_fwd(const void *q, const void *k, const void *v, void *o, float *lse, int64_t B, int H, int Sq,
                              int64_t q_sb, int64_t q_ss, int64_t k_sb, int64_t k_ss, int64_t v_sb, int64_t v_ss,
                              float scale, float p_drop, uint64_t seed, const uint64_t *seed_state, void *stream) {
    Params P;
    if (!o || !lse || !aligned16(o) || !fill(P, q, k, v, B, H, Sq, q_sb, q_ss, k_sb, k_ss, v_sb, v_ss, scale, p_drop, seed, seed_state))
        return G2048_EINVAL;
    const int64_t pairs = B * H;
    if (Sq == SK && use_mfma17())
        // heads per wave: measured at 2048 boards x 8 heads inside the update's graph, 3 launches: 8 / 4 / 2 / 1 heads per wave =
        // 69.8 / 59.6 / 61.2 / 53.6 us (the backward, then at two waves per SIMD, was flat: 128.7 / 131.5 / 133.1 / 135.1; see k_attn_bwd17_mfma)
        hipLaunchKernelGGL(small_indices(pairs) ? k_attn_fwd17_mfma<true> : k_attn_fwd17_mfma<false>,
                           dim3((unsigned)(B * (H % 8 == 0 ? 8 : (H % 2 == 0 ? 2 : 1)))), dim3(64), 0, (hipStream_t)stream, P, (uint16_t *)o, lse);
    else if (Sq == SK)
        hipLaunchKernelGGL(k_attn_fwd17, dim3((unsigned)((pairs + PAIRS - 1) / PAIRS)), dim3(64), 0, (hipStream_t)stream, P,
                           (uint16_t *)o, lse);
    else if (H == 8 && use_mfma17())
        hipLaunchKernelGGL(k_attn_fwd1_rows, dim3((unsigned)((B + 7) / 8)), dim3(256), 0, (hipStream_t)stream, P, (uint16_t *)o, lse);
    else
        hipLaunchKernelGGL(k_attn_fwd1, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream, P,
                           (uint16_t *)o, lse);
    return launch_status();
}

extern "C" int g2048_attn_bwd(const void *q, const void *k, const void *v, const void *dout, const float *lse, void *dq,
                              void *dk, void *dv, int64_t B, int H, int Sq, int64_t q_sb, int64_t q_ss, int64_t k_sb,
                              int64_t k_ss, int64_t v_sb, int64_t v_ss, float scale, float p_drop, uint64_t seed,
                              const uint64_t *seed_state, void *stream) {
    Params P;
    if (!dout || !lse || !dq || !dk || !dv || !aligned16(dout, dq, dk, dv) ||
        !fill(P, q, k, v, B, H, Sq, q_sb, q_ss, k_sb, k_ss, v_sb, v_ss, scale, p_drop, seed, seed_state))
        return G2048_EINVAL;
    const int64_t pairs = B * H;
    if (Sq == SK && use_mfma17())
        hipLaunchKernelGGL(small_indices(pairs) ? k_attn_bwd17_mfma<true> : k_attn_bwd17_mfma<false>, dim3((unsigned)pairs),
                           dim3(64), 0, (hipStream_t)stream, P, (const uint16_t *)dout, lse, (uint16_t *)dq, (uint16_t *)dk, (uint16_t *)dv);
    else if (Sq == SK)
        hipLaunchKernelGGL(k_attn_bwd17, dim3((unsigned)((pairs + PAIRS - 1) / PAIRS)), dim3(64), 0, (hipStream_t)stream, P,
                           (const uint16_t *)dout, lse, (uint16_t *)dq, (uint16_t *)dk, (uint16_t *)dv);
    else if (H == 8 && use_mfma17())
        hipLaunchKernelGGL(k_attn_bwd1_rows, dim3((unsigned)((B + 7) / 8)), dim3(256), 0, (hipStream_t)stream, P,
                           (const uint16_t *)dout, lse, (uint16_t *)dq, (uint16_t *)dk, (uint16_t *)dv);
    else
        hipLaunchKernelGGL(k_attn_bwd1, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream, P,
                           (const uint16_t *)dout, lse, (uint16_t *)dq, (uint16_t *)dk, (uint16_t *)dv);
    return launch_status();
}
