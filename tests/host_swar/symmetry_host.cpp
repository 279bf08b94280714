// Host build of 2048-ppo-agent_amd/csrc/g2048_symmetry.h (G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: lets tests/ check the per-lane canonical-frame code the kernels of g2048_symmetry.hip run against
// the numpy restatement without a GPU.  The product never builds or loads this.
#define G2048_HOST_TEST 1
#include "g2048_symmetry.h"
using namespace g2048;

extern "C" {
// the body of k_sym_canon, row by row (in place when the pointers coincide); actions / masks / frame may be null
void hst_sym_canon(const uint8_t *boards, const uint8_t *actions, const uint8_t *masks, int64_t B, uint8_t *out_boards,
                   uint8_t *out_actions, uint8_t *out_masks, uint8_t *frame) {
    for (int64_t i = 0; i < B; ++i) {
        Board bd;
        memcpy(bd.r, boards + 16 * i, 16);
        const u32 a = actions ? actions[i] : 0u, m = masks ? masks[i] : 0u;
        const u32 g = sym_canon(bd);
        memcpy(out_boards + 16 * i, bd.r, 16);
        if (out_actions) out_actions[i] = (uint8_t)sym_sigma(g, a & 3u);
        if (out_masks) out_masks[i] = (uint8_t)sym_perm_mask(g, m);
        if (frame) frame[i] = (uint8_t)g;
    }
}
// the body of k_sym_logits on 32-bit patterns
void hst_sym_logits(const uint32_t *logits, const uint8_t *frame, int64_t B, uint32_t *out) {
    for (int64_t i = 0; i < B; ++i) {
        const u32 x = logits[4 * i], y = logits[4 * i + 1], z = logits[4 * i + 2], w = logits[4 * i + 3], g = frame[i] & 7u;
        for (u32 a = 0; a < 4; ++a) out[4 * i + a] = sym_pick(x, y, z, w, sym_sigma(g, a));
    }
}
}
