// Canonical frame (include/g2048.h, "canonical frame"): the two byte movers around the policy forward.
//
//   canon   boards -> the lexicographically largest of their eight dihedral views + which view it is (the frame), and the
//           action and legal mask of the row turned into that view
//   logits  the network's four logits in the canonical frame -> the env's frame
//
// The views, the order and the permutations are in g2048_symmetry.h; the board layout and the transpose are the engine's own
// (g2048_device.h).  One lane per board: canon reads 16 B (+ 2 B) and writes 16 B (+ 3 B), logits reads 17 B and writes 16 B,
// consecutive lanes to consecutive rows (1 KiB per wave-instruction for the 16-byte accesses).  No LDS, no atomics.  Every lane
// reads all of its row before it writes any of it, and no lane touches another lane's row, so every output may be its input.
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
constexpr int64_t kMaxRows = (int64_t)1 << 30;  // a rollout buffer holds ~10 M rows; 2^30 / 256 blocks fit one grid dimension

__global__ void __launch_bounds__(kBlock) k_sym_canon(const uint8_t *boards, const uint8_t *actions, const uint8_t *masks, int64_t B,
                                                      uint8_t *out_boards, uint8_t *out_actions, uint8_t *out_masks, uint8_t *frame) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    Board bd = load_board(boards, i);
    const u32 a = actions ? actions[i] : 0u, m = masks ? masks[i] : 0u;
    const u32 g = sym_canon(bd);
    store_board(out_boards, i, bd);
    if (out_actions) out_actions[i] = (uint8_t)sym_sigma(g, a & 3u);
    if (out_masks) out_masks[i] = (uint8_t)sym_perm_mask(g, m);
    if (frame) frame[i] = (uint8_t)g;
}

__global__ void __launch_bounds__(kBlock) k_sym_logits(const float *logits, const uint8_t *frame, int64_t B, float *out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    const uint4 v = reinterpret_cast<const uint4 *>(logits)[i];  // bit patterns: moved, never recomputed
    const u32 g = frame[i] & 7u;
    reinterpret_cast<uint4 *>(out)[i] =
        make_uint4(sym_pick(v.x, v.y, v.z, v.w, sym_sigma(g, 0u)), sym_pick(v.x, v.y, v.z, v.w, sym_sigma(g, 1u)),
                   sym_pick(v.x, v.y, v.z, v.w, sym_sigma(g, 2u)), sym_pick(v.x, v.y, v.z, v.w, sym_sigma(g, 3u)));
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int g2048_sym_canon(const uint8_t *boards, const uint8_t *actions, const uint8_t *masks, int64_t B, uint8_t *out_boards,
                    uint8_t *out_actions, uint8_t *out_masks, uint8_t *frame, void *stream) {
    if (!boards || !out_boards || B <= 0 || B > kMaxRows) return G2048_EINVAL;
    if (!actions != !out_actions || !masks != !out_masks) return G2048_EINVAL;
    if (!aligned16(boards, out_boards)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_sym_canon, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, boards, actions, masks, B, out_boards,
                       out_actions, out_masks, frame);
    return launch_status();
}

int g2048_sym_logits(const float *logits, const uint8_t *frame, int64_t B, float *out, void *stream) {
    if (!logits || !frame || !out || B <= 0 || B > kMaxRows) return G2048_EINVAL;
    if (!aligned16(logits, out)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_sym_logits, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, logits, frame, B, out);
    return launch_status();
}

}  // extern "C"
