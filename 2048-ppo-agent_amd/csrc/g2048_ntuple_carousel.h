// Per-lane code of carousel shaping for the n-tuple trainer (include/g2048.h, "n-tuple carousel"): per carousel stage a pool of
// boards at which games entered that stage, and episode starts that go round the stages.
//
//   cs(x)    = #{ i : max over the 16 cells of x >= k_i }          (nt_stage over the carousel's own thresholds, all of them)
//   record   : an env whose episode goes on (flag 1) and whose board has s = cs(board) > reached: the board and its mask go to
//              slot (s - 1, b), reached = s.  Only that slot, also when s jumps by more than one.
//   restart  : an env whose episode has just ended (flag 2): turn += 1 (u32 wrap), c = (u32)(b + turn) % (n + 1).  c >= 1 draws a
//              donor j = bits(split(sub, B)[b]) % B and, if slot (c - 1, j) holds a board (mask != 0), starts there: board and
//              mask copied, reached = c.  Otherwise the engine's fresh board stays and reached = 0.  starts[stage] += 1.
//
// Slot (i, b) of pool_boards u8[n][B][16] / pool_masks u8[n][B] is at i B + b: with n <= 7 and B <= 2^28 below 2^31.  record writes
// the env's own slots and restart writes no slot, so neither launch races with itself; the kernel boundary orders them.  Integer
// arithmetic only: the device, the host build (G2048_HOST_TEST) and the numpy restatement of tests/ agree bit for bit.
#pragma once
#include "g2048_ntuple.h"

namespace g2048 {

enum { CSL_MAX_TILES = NT_MAX_STAGES - 1, CSL_NO_START = 0xFF };

// board i of a packed u8[.][16] array: the 16-byte vector access on the device, a copy in the host build
#if defined(__HIPCC__) && !defined(G2048_HOST_TEST)
#define G2048_CSL_DEV __device__ __forceinline__
G2048_CSL_DEV Board csl_load(const uint8_t *p, int64_t i) { return load_board(p, i); }
G2048_CSL_DEV void csl_store(uint8_t *p, int64_t i, const Board &b) { store_board(p, i, b); }
#else
#define G2048_CSL_DEV static inline
G2048_CSL_DEV Board csl_load(const uint8_t *p, int64_t i) {
    Board b;
    memcpy(b.r, p + 16 * i, 16);
    return b;
}
G2048_CSL_DEV void csl_store(uint8_t *p, int64_t i, const Board &b) { memcpy(p + 16 * i, b.r, 16); }
#endif

// the carousel's thresholds as the network struct nt_stage reads: n_tiles in 1 .. 7, each in 1 .. 17, strictly ascending
inline bool csl_read_tiles(const uint8_t *carousel_tiles, int n_tiles, NtNet &net) {
    memset(&net, 0, sizeof(net));
    return n_tiles >= 1 && n_tiles <= CSL_MAX_TILES && nt_read_stages(carousel_tiles, n_tiles + 1, net);
}

// env b of the record launch (flag[b] == 1)
G2048_CSL_DEV void csl_record_lane(int64_t b, int64_t B, const NtNet &net, const uint8_t *boards, const uint8_t *masks, uint8_t *reached,
                                   uint8_t *pool_boards, uint8_t *pool_masks) {
    const Board bd = csl_load(boards, b);
    const u32 s = nt_stage(net, bd);
    if (s > reached[b]) {
        const int64_t slot = (int64_t)(s - 1u) * B + b;
        csl_store(pool_boards, slot, bd);
        pool_masks[slot] = masks[b];
        reached[b] = (uint8_t)s;
    }
}

// env b of the restart launch (flag[b] == 2); returns the stage the new episode starts in (0: the engine's fresh board)
template <int MODE>
G2048_CSL_DEV u32 csl_restart_lane(u32 sub0, u32 sub1, int64_t b, int64_t B, u32 n_tiles, const uint8_t *pool_boards,
                                   const uint8_t *pool_masks, uint8_t *boards, uint8_t *masks, uint8_t *reached, u32 *turn,
                                   int64_t *starts) {
    const u32 tn = turn[b] + 1u;
    turn[b] = tn;
    const u32 c = ((u32)b + tn) % (n_tiles + 1u);
    u32 stage = 0;
    if (c) {
        u32 k0, k1;
        split_at<MODE>(sub0, sub1, (u32)B, (u32)b, k0, k1);
        const u32 j = bits_scalar<MODE>(k0, k1) % (u32)B;
        const int64_t slot = (int64_t)(c - 1u) * B + j;
        const uint8_t m = pool_masks[slot];
        if (m) {
            csl_store(boards, b, csl_load(pool_boards, slot));
            masks[b] = m;
            stage = c;
        }
    }
    reached[b] = (uint8_t)stage;
    nt_add_i64(starts + stage, 1);
    return stage;
}

}  // namespace g2048
