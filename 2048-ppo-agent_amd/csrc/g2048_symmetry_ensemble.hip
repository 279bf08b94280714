// Eight-view ensemble (include/g2048.h, "eight-view ensemble"): the two byte movers around the policy forward.
//
//   views   boards [B] -> all eight dihedral views of every board, [B][8][16]: the rows of one forward
//   fold    that forward's logits [8 B][4] and values [8 B] -> per board the mean over the views, the logits taken at the
//           action that does in the view what a does in the env's frame
//
// The views, the action map and the order-free mean are in g2048_symmetry.h.  views: one lane per OUTPUT row r = 8 b + g (as
// k_lookahead_children: the 64 lanes of a wave store one contiguous KiB, the eight lanes of a board load the same 16 bytes,
// which one cache line serves).  fold: one lane per board, 8 x 16 B + 8 x 4 B read, 16 B + 4 B written; the 16-byte loads of
// consecutive lanes lie 128 bytes apart.  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_symmetry.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBoards = (int64_t)1 << 27;  // 8 B rows: 2^30, the row limit of g2048_sym_canon

__global__ void __launch_bounds__(kBlock) k_sym_views(const uint8_t *boards, int64_t rows, uint8_t *views) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    const Board m = load_board(boards, r >> 3);
    store_board(views, r, sym_view(m, (u32)r & 7u));
}

__device__ __forceinline__ u32 component(const uint4 &v, u32 i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

__global__ void __launch_bounds__(kBlock) k_sym_fold(const float *logits, const float *values, int64_t B, float *out_logits,
                                                     float *out_values) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    if (logits) {
        uint4 row[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) row[g] = reinterpret_cast<const uint4 *>(logits)[8 * b + g];
        u32 o[4];
#pragma unroll
        for (u32 a = 0; a < 4; ++a) {
            u32 x[8];
#pragma unroll
            for (u32 g = 0; g < 8; ++g) x[g] = component(row[g], sym_sigma(g, a));  // (g, a are constants here: no select is left)
            o[a] = sym_sorted_mean8(x);
        }
        reinterpret_cast<uint4 *>(out_logits)[b] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    if (values) {
        const u32 *v = reinterpret_cast<const u32 *>(values) + 8 * b;
        u32 x[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) x[g] = v[g];
        reinterpret_cast<u32 *>(out_values)[b] = sym_sorted_mean8(x);
    }
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int g2048_sym_views(const uint8_t *boards, int64_t B, uint8_t *views, void *stream) {
    if (!boards || !views || B <= 0 || B > kMaxBoards) return G2048_EINVAL;
    if (!aligned16(boards, views)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_sym_views, dim3(blocks_for(8 * B)), dim3(kBlock), 0, (hipStream_t)stream, boards, 8 * B, views);
    return launch_status();
}

int g2048_sym_fold(const float *logits, const float *values, int64_t B, float *out_logits, float *out_values, void *stream) {
    if (!logits != !out_logits || !values != !out_values || (!logits && !values)) return G2048_EINVAL;
    if (B <= 0 || B > kMaxBoards) return G2048_EINVAL;
    if (!aligned16(logits, out_logits) || ((uintptr_t)values & 3) || ((uintptr_t)out_values & 3)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_sym_fold, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, logits, values, B, out_logits, out_values);
    return launch_status();
}

}  // extern "C"
