// Carousel shaping for the n-tuple trainer (include/g2048.h, "n-tuple carousel"): the two launches a lock-step adds after link.
//
//   record   one lane per env: an env whose episode goes on and whose board has entered a higher carousel stage than the episode
//            had reached puts the board (16 B) and its mask into its own slot of that stage's pool.  17 B in, at most 18 B out.
//   restart  one lane per env: an env whose episode has just ended takes its turn on the carousel, draws a donor env from its act
//            sub-key and copies the donor's pool board of the turn's stage over the engine's fresh board, if there is one; one
//            64-bit atomic add on the per-stage start counter.  The kernel boundary orders it after record: it reads the pools
//            including what this lock-step's record wrote, so the two are never one launch.
//
// Both are a few bytes per env: at the trainer's sizes they cost their launch.  The per-lane code is g2048_ntuple_carousel.h,
// shared with the host build the CPU tests compare against the numpy restatement.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_carousel.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBoards = (int64_t)1 << 28;

__global__ void __launch_bounds__(kBlock) k_nt_carousel_record(const uint8_t *boards, const uint8_t *masks, const uint8_t *flag,
                                                               int64_t B, const NtNet net, uint8_t *reached, uint8_t *pool_boards,
                                                               uint8_t *pool_masks) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B || flag[b] != 1) return;
    csl_record_lane(b, B, net, boards, masks, reached, pool_boards, pool_masks);
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_nt_carousel_restart(u32 sub0, u32 sub1, const uint8_t *flag, int64_t B, u32 n_tiles,
                                                                const uint8_t *pool_boards, const uint8_t *pool_masks,
                                                                uint8_t *boards, uint8_t *masks, uint8_t *reached, u32 *turn,
                                                                int64_t *starts, uint8_t *start_stage) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    u32 stage = CSL_NO_START;
    if (flag[b] == 2)
        stage = csl_restart_lane<MODE>(sub0, sub1, b, B, n_tiles, pool_boards, pool_masks, boards, masks, reached, turn, starts);
    if (start_stage) start_stage[b] = (uint8_t)stage;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline bool bad_mode(int m) { return m != G2048_RNG_LEGACY && m != G2048_RNG_PARTITIONABLE; }

}  // namespace

extern "C" {

int g2048_ntuple_carousel_record(const uint8_t *boards, const uint8_t *masks, const uint8_t *flag, int64_t B,
                                 const uint8_t *carousel_tiles, int n_tiles, uint8_t *reached, uint8_t *pool_boards,
                                 uint8_t *pool_masks, void *stream) {
    NtNet net;
    if (!boards || !masks || !flag || !carousel_tiles || !reached || !pool_boards || !pool_masks || B < 1 || B > kMaxBoards ||
        !csl_read_tiles(carousel_tiles, n_tiles, net))
        return G2048_EINVAL;
    if (!aligned16(boards, pool_boards)) return G2048_EINVAL;
    hipLaunchKernelGGL(k_nt_carousel_record, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, boards, masks, flag, B, net,
                       reached, pool_boards, pool_masks);
    return launch_status();
}

int g2048_ntuple_carousel_restart(uint32_t sub0, uint32_t sub1, const uint8_t *flag, int64_t B, int n_tiles,
                                  const uint8_t *pool_boards, const uint8_t *pool_masks, uint8_t *boards, uint8_t *masks,
                                  uint8_t *reached, uint32_t *turn, int64_t *starts, uint8_t *start_stage, int rng_mode, void *stream) {
    if (!flag || !pool_boards || !pool_masks || !boards || !masks || !reached || !turn || !starts || B < 1 || B > kMaxBoards ||
        n_tiles < 1 || n_tiles > CSL_MAX_TILES || bad_mode(rng_mode))
        return G2048_EINVAL;
    if (!aligned16(boards, pool_boards) || ((uintptr_t)turn & 3) || ((uintptr_t)starts & 7)) return G2048_EINVAL;
    if (rng_mode)
        hipLaunchKernelGGL(k_nt_carousel_restart<RNG_PARTITIONABLE>, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, sub0,
                           sub1, flag, B, (u32)n_tiles, pool_boards, pool_masks, boards, masks, reached, turn, starts, start_stage);
    else
        hipLaunchKernelGGL(k_nt_carousel_restart<RNG_LEGACY>, dim3(blocks_for(B)), dim3(kBlock), 0, (hipStream_t)stream, sub0, sub1,
                           flag, B, (u32)n_tiles, pool_boards, pool_masks, boards, masks, reached, turn, starts, start_stage);
    return launch_status();
}

}  // extern "C"
