// One-ply expectimax over the critic (include/g2048.h, "lookahead"): the three kernels around the value forward.
//
//   expand    boards -> the four afterstates, their merge scores and the number of spawn children behind each
//   children  afterstates -> every (empty cell, tile 2 / tile 4) child, packed in (b, a, cell, tile) order
//   reduce    values of the children -> Q(s, a) = r + gamma * mean over cells of (0.9 V(2-child) + 0.1 V(4-child))
//
// The slide/merge and legality rules are the engine's own (g2048_device.h): nothing here restates them.  All three are byte
// movers: per board expand reads 16 B and writes 96 B, children writes 17 B per child (at most 120 children per board,
// a few dozen in play), reduce reads 5 B per child.  No LDS, no atomics; the children are written with vector stores,
// one 16-byte store per lane, consecutive lanes to consecutive rows (1 KiB per wave-instruction).
//
// Two plies (include/g2048.h, "two-ply") run the same three kernels on both levels and add two between them:
//
//   dedup     the afterstates of one root's (child, action) pairs -> the first pair with the same 16 bytes, per root
//   backup    level-2 expectations -> V1 of every level-1 child, the max over its legal actions
//
// dedup is the only kernel here with LDS: one workgroup per root stages the root's keys (at most 480 x 16 B) and every lane
// scans the keys before its own pair.  backup is a byte mover like the others (48 B read, 4 gathers, 4 B written per child).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBoards = (int64_t)1 << 24;    // 4 * B * 30 children stay below 2^31: the offsets are int32
constexpr int64_t kMaxChildren = (int64_t)1 << 31;  // exclusive

// bit 7 of every EMPTY byte of a row
__device__ __forceinline__ u32 empty_bits(u32 row) { return tile_bits(row) ^ 0x80808080u; }

// One lane per board: one 16-byte load, four board_moves (the direction is a compile-time constant after unrolling, so the
// selects inside board_move fold away), 4 x 16 B + 16 B + 16 B of stores.
__global__ void __launch_bounds__(kBlock) k_lookahead_expand(const uint8_t *boards, int64_t B, uint8_t *after, float *reward,
                                                             int32_t *nchild) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    const Board bd = load_board(boards, i);
    const u32 legal = board_legal(bd);
    float r[4];
    int32_t n[4];
#pragma unroll
    for (u32 a = 0; a < 4; ++a) {
        Board nb = bd;
        const u32 score = board_move(nb, a);
        const bool ok = (legal >> a) & 1u;
        u32 empties = 0;
        for (int k = 0; k < 4; ++k) {
            nb.r[k] = ok ? nb.r[k] : bd.r[k];
            empties += popc(empty_bits(nb.r[k]));
        }
        store_board(after, 4 * i + a, nb);
        r[a] = ok ? (float)score : 0.0f;
        n[a] = ok ? (int32_t)(2u * empties) : 0;
    }
    reinterpret_cast<float4 *>(reward)[i] = make_float4(r[0], r[1], r[2], r[3]);
    reinterpret_cast<int4 *>(nchild)[i] = make_int4(n[0], n[1], n[2], n[3]);
}

// One lane per CHILD.  Lane c finds its (b, a) pair p by a binary search in offset (the last p with offset[p] <= c: pairs
// without children share their successor's offset and are skipped by taking the last), then j = c - offset[p] selects the
// (j / 2)-th empty cell of the afterstate in ascending cell index and the tile 1 + (j & 1).  The 64 lanes of a wave cover at
// most a few pairs, so the search and the afterstate load hit the same cache lines in every lane; the store is one
// contiguous KiB per wave.  Lanes whose inputs disagree (j past nchild[p], fewer empty cells than claimed) write nothing.
__global__ void __launch_bounds__(kBlock) k_lookahead_children(const uint8_t *after, const int32_t *nchild, const int32_t *offset,
                                                               int64_t P /* = 4 B pairs */, int64_t N, uint8_t *children,
                                                               uint8_t *terminal) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= N) return;
    int64_t lo = 0, hi = P - 1;  // invariant: offset[lo] <= c (offset[0] == 0)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)offset[mid] <= c) lo = mid;
        else hi = mid - 1;
    }
    const int64_t j = c - (int64_t)offset[lo];
    if (j < 0 || j >= (int64_t)nchild[lo]) return;
    Board bd = load_board(after, lo);
    // the (j / 2)-th empty cell, row-major: row by running totals, column inside the row (as board_spawn does)
    const u32 k = (u32)(j >> 1) + 1u;  // 1-based
    u32 z[4], cum[4];
    for (int q = 0; q < 4; ++q) z[q] = empty_bits(bd.r[q]);
    cum[0] = popc(z[0]);
    cum[1] = cum[0] + popc(z[1]);
    cum[2] = cum[1] + popc(z[2]);
    cum[3] = cum[2] + popc(z[3]);
    if (k > cum[3]) return;
    const u32 row = (u32)(k > cum[0]) + (u32)(k > cum[1]) + (u32)(k > cum[2]);
    const u32 before = row == 0 ? 0u : (row == 1 ? cum[0] : (row == 2 ? cum[1] : cum[2]));
    const u32 zr = row == 0 ? z[0] : (row == 1 ? z[1] : (row == 2 ? z[2] : z[3]));
    const u32 kk = k - before;
    const u32 f0 = (zr >> 7) & 1u, f1 = f0 + ((zr >> 15) & 1u), f2 = f1 + ((zr >> 23) & 1u);
    const u32 col = (u32)(kk > f0) + (u32)(kk > f1) + (u32)(kk > f2);
    const u32 val = (1u + ((u32)j & 1u)) << (8u * col);  // the cell is empty: OR places the tile
    for (int q = 0; q < 4; ++q) bd.r[q] |= (row == (u32)q) ? val : 0u;
    store_board(children, c, bd);
    terminal[c] = board_legal(bd) == 0 ? 1 : 0;
}

// One lane per (b, a).  offset[p] is even (a sum of even counts), so the pair (V(2-child), V(4-child)) of one cell is one
// aligned 8-byte load and its two terminal flags one 2-byte load.  Ascending j, f32, products and sums rounded one by one.
__global__ void __launch_bounds__(kBlock) k_lookahead_reduce(const float *reward, const int32_t *nchild, const int32_t *offset,
                                                             const float *values, const uint8_t *terminal, float gamma, int64_t P,
                                                             int64_t N, float *q) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const int32_t n = nchild[p];
    const int64_t o = offset[p];
    if (n <= 0 || (n & 1) || (o & 1) || o < 0 || o + n > N) {  // no children (or inconsistent inputs): the mask removes the action
        q[p] = 0.0f;
        return;
    }
    const int ne = n >> 1;
    const float2 *v2 = reinterpret_cast<const float2 *>(values + o);
    const uchar2 *t2 = reinterpret_cast<const uchar2 *>(terminal + o);
    float acc = 0.0f;
    for (int j = 0; j < ne; ++j) {
        const float2 v = v2[j];
        const uchar2 t = t2[j];
        const float a = t.x ? 0.0f : v.x, b = t.y ? 0.0f : v.y;
        acc = add_rn(acc, add_rn(mul_rn(0.9f, a), mul_rn(0.1f, b)));
    }
    q[p] = add_rn(reward[p], mul_rn(gamma, acc / (float)ne));
}

// One workgroup per root.  The keys are staged linearly, 16 B per pair: in the scan every lane of a wave reads the SAME key q
// (one ds_read_b128 whose 64 addresses are identical broadcasts, so no layout can conflict), compares it with its own key in
// registers and stops at its first match; a wave runs to the longest scan among its lanes.  A pair without children is staged
// as a key no board has (0xFF in every cell), so it matches nothing and nothing matches it.  Each pair is written by exactly one
// lane and read-only state decides what it writes: no atomics, no dependence on scheduling.  A group whose bounds disagree
// (negative, past P, more than kMaxGroup pairs) gets rep = p, nuniq = 0 on the part of its range inside [0, P): no child of it
// is valued, its actions back up 0; a decreasing pair of bounds writes nothing.
constexpr int kDedupBlock = 128;
constexpr int kMaxGroup = 480;  // 120 level-1 children x 4 actions

__global__ void __launch_bounds__(kDedupBlock) k_lookahead_dedup(const uint8_t *after, const int32_t *nchild, const int32_t *group_start,
                                                                 int64_t P, int32_t *rep, int32_t *nuniq) {
    __shared__ uint4 keys[kMaxGroup];
    const int64_t s = group_start[blockIdx.x], e = group_start[blockIdx.x + 1];
    if (s < 0 || e < s || e > P || e - s > kMaxGroup) {  // uniform over the block: nobody waits at the barrier below
        // benign on inconsistent bounds: what of the range lies inside [0, P) is left without duplicates and without children
        const int64_t lo = s < 0 ? 0 : s, hi = e > P ? P : e;
        for (int64_t i = lo + threadIdx.x; i < hi; i += kDedupBlock) {
            rep[i] = (int32_t)i;
            nuniq[i] = 0;
        }
        return;
    }
    const int n = (int)(e - s);
    uint4 mine[(kMaxGroup + kDedupBlock - 1) / kDedupBlock];
    int32_t cnt[(kMaxGroup + kDedupBlock - 1) / kDedupBlock];
#pragma unroll
    for (int k = 0; k < (kMaxGroup + kDedupBlock - 1) / kDedupBlock; ++k) {
        const int i = k * kDedupBlock + (int)threadIdx.x;
        if (i < n) {
            cnt[k] = nchild[s + i];
            mine[k] = cnt[k] > 0 ? reinterpret_cast<const uint4 *>(after)[s + i] : make_uint4(~0u, ~0u, ~0u, ~0u);
            keys[i] = mine[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (kMaxGroup + kDedupBlock - 1) / kDedupBlock; ++k) {
        const int i = k * kDedupBlock + (int)threadIdx.x;
        if (i >= n) continue;
        int first = i;
        if (cnt[k] > 0) {
            for (int q = 0; q < i; ++q) {
                const uint4 o = keys[q];
                // one 128-bit read and a branch-free compare (&& would fetch the key a dword at a time)
                if (((o.x ^ mine[k].x) | (o.y ^ mine[k].y) | (o.z ^ mine[k].z) | (o.w ^ mine[k].w)) == 0u) {
                    first = q;
                    break;
                }
            }
        }
        rep[s + i] = (int32_t)(s + first);
        nuniq[s + i] = first == i ? cnt[k] : 0;
    }
}

// One lane per level-1 child: its four rewards, counts and representatives are one 16-byte load each, the expectations four
// gathers.  A representative outside [0, P) (inconsistent inputs) removes the action like a count of 0 does.
__global__ void __launch_bounds__(kBlock) k_lookahead_backup(const float *reward, const int32_t *nchild, const int32_t *rep,
                                                             const float *e, int64_t N1, float *v1) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= N1) return;
    const float4 r4 = reinterpret_cast<const float4 *>(reward)[c];
    const int4 n4 = reinterpret_cast<const int4 *>(nchild)[c];
    const int4 p4 = reinterpret_cast<const int4 *>(rep)[c];
    const float r[4] = {r4.x, r4.y, r4.z, r4.w};
    const int32_t n[4] = {n4.x, n4.y, n4.z, n4.w}, p[4] = {p4.x, p4.y, p4.z, p4.w};
    bool any = false;
    float best = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (n[a] <= 0 || p[a] < 0 || (int64_t)p[a] >= 4 * N1) continue;
        const float x = add_rn(r[a], e[p[a]]);
        best = (!any || x > best) ? x : best;
        any = true;
    }
    v1[c] = best;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int g2048_lookahead_expand(const uint8_t *boards, int64_t B, uint8_t *after, float *reward, int32_t *nchild, void *stream) {
    if (!boards || !after || !reward || !nchild || B <= 0 || B > kMaxBoards) return G2048_EINVAL;
    if (!aligned16(boards, after, reward, nchild)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_lookahead_expand, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, boards, B, after, reward, nchild);
    return launch_status();
}

int g2048_lookahead_children(const uint8_t *after, const int32_t *nchild, const int32_t *offset, int64_t B, int64_t N,
                             uint8_t *children, uint8_t *terminal, void *stream) {
    if (!after || !nchild || !offset || B <= 0 || B > kMaxBoards || N < 0 || N >= kMaxChildren || N > 120 * B) return G2048_EINVAL;
    if (N == 0) return 0;
    if (!children || !terminal || !aligned16(after, children) || ((uintptr_t)nchild & 3) || ((uintptr_t)offset & 3)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_lookahead_children, dim3(blocks_for(N)), dim3(kBlock), 0, (hipStream_t)stream, after, nchild, offset, 4 * B, N,
                       children, terminal);
    return launch_status();
}

int g2048_lookahead_reduce(const float *reward, const int32_t *nchild, const int32_t *offset, const float *values,
                           const uint8_t *terminal, double gamma, int64_t B, int64_t N, float *q, void *stream) {
    if (!reward || !nchild || !offset || !q || B <= 0 || B > kMaxBoards || N < 0 || N >= kMaxChildren || N > 120 * B) return G2048_EINVAL;
    if (N > 0 && (!values || !terminal)) return G2048_EINVAL;
    if (((uintptr_t)reward & 3) || ((uintptr_t)nchild & 3) || ((uintptr_t)offset & 3) || ((uintptr_t)q & 3) || ((uintptr_t)values & 7) ||
        ((uintptr_t)terminal & 1))
        return G2048_EINVAL;
    hipLaunchKernelGGL(k_lookahead_reduce, dim3(blocks_for(4 * B)), dim3(kBlock), 0, (hipStream_t)stream, reward, nchild, offset, values,
                       terminal, (float)gamma, 4 * B, N, q);
    return launch_status();
}

int g2048_lookahead_dedup(const uint8_t *after, const int32_t *nchild, const int32_t *group_start, int64_t G, int64_t P, int32_t *rep,
                          int32_t *nuniq, void *stream) {
    if (!after || !nchild || !group_start || !rep || !nuniq || G <= 0 || G > kMaxBoards || P < 0 || P > 4 * kMaxBoards ||
        P > kMaxGroup * G || (P & 3))
        return G2048_EINVAL;
    if (!aligned16(after) || ((uintptr_t)nchild & 3) || ((uintptr_t)group_start & 3) || ((uintptr_t)rep & 3) || ((uintptr_t)nuniq & 3))
        return G2048_EINVAL;
    if (P == 0) return 0;
    hipLaunchKernelGGL(k_lookahead_dedup, dim3((unsigned)G), dim3(kDedupBlock), 0, (hipStream_t)stream, after, nchild, group_start, P, rep,
                       nuniq);
    return launch_status();
}

int g2048_lookahead_backup(const float *reward, const int32_t *nchild, const int32_t *rep, const float *e, int64_t N1, float *v1,
                           void *stream) {
    if (!reward || !nchild || !rep || !e || !v1 || N1 <= 0 || N1 > kMaxBoards) return G2048_EINVAL;
    if (!aligned16(reward, nchild, rep) || ((uintptr_t)e & 3) || ((uintptr_t)v1 & 3)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_lookahead_backup, dim3(blocks_for(N1)), dim3(kBlock), 0, (hipStream_t)stream, reward, nchild, rep, e, N1, v1);
    return launch_status();
}

}  // extern "C"
