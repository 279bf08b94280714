/*
 * g2048.h -- C ABI of libg2048.so, the MI355X (gfx950) 2048 rollout engine.
 *
 * This is the drop-in boundary of the hot path.  The reference (michaelriedl/2048-ppo-agent) is pure
 * Python and has no FFI of its own: its hot path calls jitted JAX/Pgx functions.  Each entry point
 * below names the reference call it replaces (paths relative to the reference repo); the ctypes
 * binding a maintainer would add is shown in INTEGRATION.md and lives in
 * 2048-ppo-agent_amd/src/g2048/native.py.
 *
 * Conventions
 *   - All array pointers are DEVICE pointers owned by the caller (e.g. torch tensors); the library
 *     never allocates, frees, copies to the host or synchronises.  Kernels are enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream).  Host-side arguments are marked (host).
 *   - Return value: 0 on success, G2048_EINVAL (-1) for a bad argument, -(1000 + hipError_t) when the
 *     launch itself failed.  Nothing throws.  Re-entrant: no global state (kernels that need more than the default
 *     dynamic-LDS limit set that per-device function attribute on every call instead of latching it).
 *   - boards   u8[B][16]  log2(tile) per cell, row-major, 0 = empty, values <= 30; 16-byte aligned
 *   - masks    u8[B]      bit a = legal_action_mask[a]  (0 left, 1 up, 2 right, 3 down)
 *   - done     u8[B]      terminated flag (0/1)
 *   - keys     u32[B][2]  one JAX threefry key per env
 *   - rng_mode 0 = legacy threefry stream (jax_threefry_partitionable=False),
 *              1 = partitionable stream (default of the reference's pinned jax 0.5.3)
 *   - Trajectories are step-major SoA with row stride B:  x[t][e] at index t*B + e
 *       tr_boards u8[T][B][16]  board BEFORE step t (the observation the policy saw)
 *       tr_meta   u8[T][B]      action | mask_before << 2 | done_after << 6
 *       tr_rewards/tr_logp/tr_values f32[T][B]
 */
#ifndef G2048_H
#define G2048_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_ABI_VERSION 4
#define G2048_EINVAL (-1)
#define G2048_RNG_LEGACY 0
#define G2048_RNG_PARTITIONABLE 1
#define G2048_POLICY_DRUL 0
#define G2048_POLICY_RANDOM 1
/* most lock-steps one g2048_rollout_fused launch can advance (its key table rides in the kernarg) */
#define G2048_MAX_FUSED_STEPS 128

int g2048_abi_version(void);

/* ---- RNG ---------------------------------------------------------------------------------------- */

/* out[j] = jax.random.split(key, n)[j].  Replaces `subkey = jax.random.split(subkey, batch_size)`
 * (src/runs/batch_runner.py:106,119,127; src/runs/run_actions_batch.py:43,50,53). */
int g2048_split(uint32_t key0, uint32_t key1, uint32_t *out_keys, int64_t n, int rng_mode, void *stream);

/* (host, no device work) n times `key, sub = jax.random.split(key)`: key[2] is advanced in place,
 * subs[i] = i-th sub-key.  Replaces the host-side chain at src/runs/batch_runner.py:105,118,126. */
int g2048_chain_keys(uint32_t *key /*host [2]*/, uint32_t *subs /*host [n][2]*/, int64_t n, int rng_mode);

/* ---- env, explicit per-env keys (the shape of the reference's vmapped calls) ----------------------- */

/* jit(vmap(env.init))(keys)           src/runs/batch_runner.py:34,107 */
int g2048_init(const uint32_t *keys, uint8_t *boards, uint8_t *masks, uint8_t *done, int64_t B,
               int rng_mode, void *stream);

/* jit(vmap(env.step))(state, action, keys), state updated in place.   src/runs/batch_runner.py:35,128
 * Algorithmic traffic: 50 B per env (board 16 r + 16 w, action 4, key 8, reward 4, mask 1, done 1). */
int g2048_step(uint8_t *boards, uint8_t *masks, uint8_t *done, const int32_t *actions,
               const uint32_t *keys, float *rewards, int64_t B, int rng_mode, void *stream);

/* State.observation: obs u8(bool)[B][4][4][31], obs[e][r][c][k] = (board == k).  Only for callers that
 * want the reference's one-hot array (src/runs/batch_runner.py:121,138); the engine never needs it. */
int g2048_observe(const uint8_t *boards, uint8_t *obs, int64_t B, void *stream);

/* ---- act_fn plug-ins, batched ------------------------------------------------------------------- */

/* src/actions/act_drul.py:40-44 */
int g2048_act_drul(const uint8_t *masks, int32_t *actions, int64_t B, void *stream);
/* src/actions/act_randomly.py:40-54 */
int g2048_act_random(const uint32_t *keys, const uint8_t *masks, int32_t *actions, float *log_probs,
                     int64_t B, int rng_mode, void *stream);
/* tail of TorchActionFunction.__call__ (src/ppo/torch_action_wrapper.py:85-102) given the agent's raw
 * actor logits f32[B][4]; use_mask applies src/ppo/ppo_agent.py:117-121 first. */
int g2048_act_logits(const uint32_t *keys, const float *logits, const uint8_t *masks, int use_mask,
                     int sample, int32_t *actions, float *log_probs, int64_t B, int rng_mode, void *stream);

/* ---- fused rollout engine (keys derived in-kernel from the batch-wide sub-key) ---------------------
 * env i of this call is global env (env0 + i) of a batch of B_total envs, so a shard reproduces exactly
 * the slice of the single-device run (keys = split(sub, B_total)[env0 + i]). */

/* init + zero ep_len.  sub = the sub-key of batch_runner.py:105-106. */
int g2048_reset_fused(uint32_t sub0, uint32_t sub1, uint8_t *boards, uint8_t *masks, uint8_t *done,
                      int32_t *ep_len, int64_t B, int64_t B_total, int64_t env0, int rng_mode, void *stream);

/* n_steps lock-steps of BatchRunner's loop body (batch_runner.py:117-136) with a fused naive policy,
 * boards resident in registers across steps.  step_subs (host) = [n_steps][4]: act sub-key, step sub-key.
 * Writes steps t0..t0+n_steps-1 of the trajectory (tr_logp may be NULL; unused for DRUL).
 * fill_frozen != 0 also writes the frozen frames of already-finished envs (what the reference's [B,T]
 * arrays contain); 0 skips them and lets finished waves retire.  ep_len[e] counts steps through the first
 * termination.  *live_count (device u32, zeroed by the caller) += envs still running afterwards. */
int g2048_rollout_fused(const uint32_t *step_subs /*host*/, int n_steps, int64_t t0, uint8_t *boards,
                        uint8_t *masks, uint8_t *done, int32_t *ep_len, uint8_t *tr_boards,
                        uint8_t *tr_meta, float *tr_rewards, float *tr_logp, int64_t B, int64_t B_total,
                        int64_t env0, int policy, int fill_frozen, int rng_mode, uint32_t *live_count,
                        void *stream);

/* One lock-step with the policy's outputs already on the device: sample (or argmax) from logits,
 * log-prob, env step, trajectory write at step t -- the fusion of batch_runner.py:123-136 with
 * torch_action_wrapper.py:85-102.  logits f32[B][4], values f32[B] come from the agent forward.
 * live_count (device u32, zeroed by the caller; may be NULL when nobody polls after this step): += envs still running
 * afterwards, one atomic per workgroup that has any. */
int g2048_policy_step(uint32_t act_sub0, uint32_t act_sub1, uint32_t step_sub0, uint32_t step_sub1,
                      const float *logits, const float *values, int use_mask, int sample, int64_t t,
                      uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len, uint8_t *tr_boards,
                      uint8_t *tr_meta, float *tr_rewards, float *tr_logp, float *tr_values, int64_t B,
                      int64_t B_total, int64_t env0, int fill_frozen, int rng_mode, uint32_t *live_count,
                      void *stream);

/* Fixed-horizon throughput mode (no reference counterpart; it replaces the lock-step `while not all terminated` of
 * src/runs/batch_runner.py:117): g2048_policy_step for EVERY lane at every call, and a lane whose step
 * terminates starts its next episode at once: state = env.init(split(fold_in(step_sub, 0xFFFFFFFF), B_total)[env0 + i]).
 * Row t of the trajectory is written as by g2048_policy_step (done_after = 1 marks the episode boundary); boards/masks hold
 * the state for step t+1 (a fresh board after a terminal step), ep_len[i] the steps of the running episode.  The key chain
 * advances exactly as in the reference (two splits per lock-step), so until a lane's first termination its rows are those
 * of the lock-step mode under the same policy outputs. */
int g2048_policy_step_autoreset(uint32_t act_sub0, uint32_t act_sub1, uint32_t step_sub0, uint32_t step_sub1,
                                const float *logits, const float *values, int use_mask, int sample, int64_t t,
                                uint8_t *boards, uint8_t *masks, int32_t *ep_len, uint8_t *tr_boards, uint8_t *tr_meta,
                                float *tr_rewards, float *tr_logp, float *tr_values, int64_t B, int64_t B_total,
                                int64_t env0, int rng_mode, void *stream);
/* (host, no device work) out[2] = jax.random.fold_in(step_sub, 0xFFFFFFFF): the per-step reset sub-key of that mode. */
int g2048_reset_key(uint32_t step_sub0, uint32_t step_sub1, uint32_t *out /*host [2]*/);

/* ---- rollout buffer + GAE ----------------------------------------------------------------------- */

/* GAE over the step-major trajectory: env e uses steps 0..ep_len[e]-1 (its last kept step is terminal).
 * Same float32 operation order as PPODataset._compute_gae_returns (src/ppo/data_loader.py:103-130),
 * so results are bit-identical to the reference's scan over the compacted buffer. 17 B per env-step. */
int g2048_gae_tb(const float *tr_rewards, const float *tr_values, const int32_t *ep_len, float *tr_adv,
                 float *tr_ret, int64_t T, int64_t B, double gamma, double lam, void *stream);

/* GAE over a fixed-horizon trajectory: all T steps of every lane, episode boundaries = the done_after bit of tr_meta (the
 * reset at `terminations[step]` of src/ppo/data_loader.py:103-130), bootstrapped from last_values[e] = V(state after step
 * T-1) where the horizon cut an episode.  Same float32 operation order as g2048_gae_tb. */
int g2048_gae_tb_boot(const float *tr_rewards, const float *tr_values, const uint8_t *tr_meta, const float *last_values,
                      float *tr_adv, float *tr_ret, int64_t T, int64_t B, double gamma, double lam, void *stream);

/* GAE over a flat buffer with termination flags (the reference's layout, data_loader.py:103-130). */
int g2048_gae_flat(const float *rewards, const float *values, const uint8_t *terms, float *adv, float *ret,
                   int64_t N, double gamma, double lam, void *stream);

/* RolloutBuffer.store_batch (src/ppo/rollout_buffer.py:164-187): keep steps 0..ep_len[e]-1 of every env,
 * env-major, at offsets[e] (exclusive prefix sum of ep_len, int64).  The optional f32 columns (log-probs, values, and
 * the advantages / returns of g2048_gae_tb computed on the coalesced [T][B] layout) may be NULL together with their
 * outputs.  out_terms[n] = 1 on each env's last kept step. */
int g2048_compact(const uint8_t *tr_boards, const uint8_t *tr_meta, const float *tr_rewards, const float *tr_logp,
                  const float *tr_values, const float *tr_adv, const float *tr_ret, const int32_t *ep_len,
                  const int64_t *offsets, uint8_t *out_boards, uint8_t *out_actions, uint8_t *out_masks, float *out_rewards,
                  float *out_logp, float *out_values, float *out_adv, float *out_ret, uint8_t *out_terms, int64_t T,
                  int64_t B, void *stream);

/* ---- policy network (inference) ------------------------------------------------------------------- */

/* Fused bf16 forward of the reference's Transformer encoder at its default shape (d_model 256, 8 heads, ff 1024,
 * 17 tokens, "cls" reduction): boards u8[B][16] -> features f32[B][256], i.e. PPOAgent's
 * `self.transformer(self.input_embedding(obs), reduction="cls")` (src/ppo/ppo_agent.py:103-106,
 * src/ppo/transformer_encoder.py:150-190) in eval mode under bf16 autocast numerics.
 *   embed_table f32[16][31][256] = input_embedding.weight^T[e] + positional code of cell c   (16-byte aligned)
 *   cls_token   f32[256]                                                                     (16-byte aligned)
 * The per-layer parameters are passed PACKED (the caller packs once per policy update; src/ppo/fused_policy.py):
 *   folding, in f32:  LayerNorm's affine goes into the Linear behind it (W' = W diag(gamma), b' = b + W beta, for
 *     norm1 -> in_proj and norm2 -> linear1); the key bias is dropped (it shifts every score of a query by the same
 *     amount, softmax does not see it); the value bias moves into out_proj's: bo' = bo + Wo bv' (softmax rows sum to 1);
 *   column order: the kernel feeds accumulator tiles straight back in as MFMA operands, so the input columns of every
 *     group of 16 of all four matrices are stored in the order [0 1 2 3 8 9 10 11 4 5 6 7 12 13 14 15];
 *   weights_bf16, per layer: in_proj_weight'[768][256] | out_proj.weight[256][256] | linear1.weight'[1024][256] |
 *                            linear2.weight[256][1024]                                     (bf16, 16-byte aligned)
 *   params_f32,  per layer: ones[256] | zeros[256] | bq'[256], zeros[512] | bo'[256] | ones[256] | zeros[256] |
 *                            b1'[1024] | linear2.bias[256]   (the slots of the folded LayerNorm affines are unused)
 *
 * workspace: NULL = one kernel carries every token through every layer.  Otherwise
 * g2048_policy_encoder_workspace_bytes(B) bytes (16-byte aligned): the last layer is split - a first kernel runs it up to
 * the CLS row's attention, a second one batches the CLS tokens of 128 boards per workgroup through the rest of it (only
 * the CLS row of the last layer is read by the "cls" reduction).  Same result up to summation order.
 * Workspace layout: the first B * 1536 bytes are used - bf16 [B][256] attention output of the CLS rows (per head the 32
 * dims in the packed weights' column order), then f32 [B][256] their residual rows; the rest is not touched.  With
 * G2048_ENCODER_KV_WS=1 in the environment (read per call; the A/B arm of the same computation, bit-identical features)
 * the whole workspace is used: bf16 [B][8 heads][17 keys][2][16] K, the same for V, then the f32 residual rows. */
int64_t g2048_policy_encoder_workspace_bytes(int64_t B);
int g2048_policy_encoder(const uint8_t *boards, const float *embed_table, const float *cls_token,
                         const void *weights_bf16, const float *params_f32, int n_layers, float *features,
                         int64_t B, void *workspace, void *stream);

/* The same encoder with the "mean" reduction, PPOAgent's default (src/ppo/ppo_agent.py:26): features f32[B][256] =
 * encoder_output[:, 1:, :].mean(dim=1), the mean over the 16 board tokens (src/ppo/transformer_encoder.py:188-190).
 * Blob formats, parameter folding and alignments as g2048_policy_encoder.  One kernel carries every token through all
 * n_layers (every token of the last layer is read, so there is no split form and no workspace); the 16 rows of a board are
 * summed in ascending token order in f32 and scaled by 1/16, so two calls give bit-identical features. */
int g2048_policy_encoder_mean(const uint8_t *boards, const float *embed_table, const float *cls_token,
                              const void *weights_bf16, const float *params_f32, int n_layers, float *features,
                              int64_t B, void *stream);

/* ---- policy network (inference, fp32 rollout): split-fp16 products on the matrix cores --------------------------------
 * The reference rolls out in fp32 (src/ppo/torch_action_wrapper.py:73-102).  These four entry points are that forward with every
 * activation between kernels f32 and every Linear of the encoder a two-way fp16 split product: v = (hi + lo) / s with
 * hi = f16(s v), lo = f16(s v - hi), three f16 MFMAs per fragment pair (lo_w hi_x, hi_w lo_x, hi_w hi_x) into one f32
 * accumulator, the result multiplied by 1 / (sx sw) in f32.  Scales are powers of two chosen by the caller with |s v| <= 2^15
 * for every element (an element beyond fp16's range gives inf / NaN outputs, not a quietly wrong number); elements with
 * |s v| >= 2^-3 keep 22 significand bits, smaller ones an absolute error of at most 2^-14 / s. */
#define G2048_F32SPLIT_BIAS 0      /* y = x W^T + b */
#define G2048_F32SPLIT_BIAS_RELU 1 /* y = relu(x W^T + b) */
#define G2048_F32SPLIT_ADD_LN 2    /* y = resid + x W^T + b;  h = LayerNorm(y) * gamma + beta   (N = 256) */
#define G2048_F32SPLIT_ADD 3       /* y = resid + x W^T + b                                     (N = 256) */

/* Weight planes of one Linear (reference: the nn.Linear / in_proj weights read by torch_action_wrapper.py:73-102 through the agent).
 * w f32 [N][K] row-major -> packed, 4 N K bytes of fp16: unit (((c K/16 + ks) 8 + nt) 2 + p) 64 + l (16 bytes each) holds plane p
 * (0 hi, 1 lo) of w[256 c + 32 nt + (l & 31)][16 ks + 8 (l >> 5) + 0..7] * scale: the matrix-core A fragment of lane l.
 * G2048_EINVAL: a null or misaligned (16 bytes) pointer, K not in {256, 1024}, N not in {256, 768, 1024}, scale not a power of two. */
int g2048_f32split_pack(const float *w, int N, int K, float scale, void *packed, void *stream);

/* One Linear of the fp32 rollout forward (torch_action_wrapper.py:73-102: in_proj, out_proj, linear1, linear2 of every encoder layer).
 * x f32 [T][K] with row stride ldx; w_packed from g2048_f32split_pack with scale sw; bias f32 [N]; y f32 [T][N] with row stride ldy;
 * epilogue one of G2048_F32SPLIT_*.  For ADD_LN / ADD: resid f32 [T][256] contiguous (y may be resid itself), and for ADD_LN gamma,
 * beta f32 [256], h f32 [T][256] contiguous, eps > 0.  sx: the power of two x is multiplied by before it is split.  Rows past T and
 * bytes outside the outputs are not written.
 * G2048_EINVAL: a null or misaligned required pointer, T < 1, unsupported K / N (as above; N = 256 for ADD_LN / ADD), ldx < K,
 * ldy < N, strides not multiples of 4, an unknown epilogue, sx or sw not a power of two. */
int g2048_f32split_gemm(const float *x, int64_t ldx, const void *w_packed, const float *bias, float *y, int64_t ldy,
                        const float *resid, const float *gamma, const float *beta, float *h, int64_t T, int K, int N,
                        int epilogue, float sx, float sw, float eps, void *stream);

/* Self-attention of the fp32 rollout forward (torch_action_wrapper.py:73-102 -> nn.TransformerEncoderLayer, eval mode: no dropout):
 * 17 tokens, H heads of 32, qkv f32 [B][17][3 * 32 H] (the packed in_proj output, read in place), o f32 [B][17][32 H];
 * softmax(scale q k^T) v in f32 FMAs.  G2048_EINVAL: a null or misaligned pointer, B < 1, H outside 1 .. 64. */
int g2048_attn_fwd_f32(const float *qkv, float *o, int64_t B, int H, float scale, void *stream);

/* Token embedding of the fp32 rollout forward (torch_action_wrapper.py:73-102 -> ppo_agent.py:59-66, transformer_encoder.py:150-190):
 * x0[b][0] = cls, x0[b][1 + c] = table[c][boards[b][c]] (table f32 [16][31][256] = positional code + embedding row), and
 * h = LayerNorm(x0) * gamma + beta (layers[0].norm1), both f32 [B][17][256].  G2048_EINVAL: a null or misaligned pointer, B < 1. */
int g2048_embed_ln_f32(const uint8_t *boards, const float *table, const float *cls, const float *gamma, const float *beta, float eps,
                       float *x0, float *h, int64_t B, void *stream);

/* ---- one-ply expectimax over the critic (no reference counterpart: the reference only ever asks the actor) -----------
 * Q(s, a) = r(s, a) + gamma * E_{s' ~ spawn(after(s, a))} V(s'), V(terminal s') = 0, with the spawn law of the env (uniform
 * over the empty cells of the afterstate, tile 2 with p = 0.9, tile 4 with p = 0.1).  Three kernels around the caller's
 * value forward: expand -> (exclusive prefix sum of nchild, by the caller) -> children -> V(children) -> reduce.
 * Pairs (b, a) are indexed p = 4 * b + a; offset i32[B][4] is the exclusive prefix sum of nchild in that order and N its
 * total (host: the caller reads it back once to size the children and the forward). */

/* after u8[B][4][16] = the board slid in direction a (the input board where the move is illegal); reward f32[B][4] = the
 * merge score g2048_step returns for that move (0 where illegal); nchild i32[B][4] = 2 * (empty cells of the afterstate)
 * where the move is legal, 0 where not.  One lane per board; 16 B read, 96 B written per board.
 * G2048_EINVAL: a null pointer, B outside 1 .. 2^24, a pointer that is not 16-byte aligned. */
int g2048_lookahead_expand(const uint8_t *boards, int64_t B, uint8_t *after, float *reward, int32_t *nchild, void *stream);

/* children u8[N][16], terminal u8[N]: the children of pair p occupy rows offset[p] .. offset[p] + nchild[p], ordered by
 * empty cell in ascending (row-major) cell index and within a cell tile 2 (log2 = 1) first, tile 4 (log2 = 2) second;
 * terminal[i] = 1 iff child i has no legal move.  One lane per child, one 16-byte store each; rows at or past N are not
 * touched, and a lane whose offset / nchild / afterstate disagree writes nothing.  N = 0 launches nothing.
 * G2048_EINVAL: a null pointer (children / terminal may be null when N = 0), B outside 1 .. 2^24, N < 0 or N > 120 * B,
 * after / children not 16-byte aligned, nchild / offset not 4-byte aligned. */
int g2048_lookahead_children(const uint8_t *after, const int32_t *nchild, const int32_t *offset, int64_t B, int64_t N,
                             uint8_t *children, uint8_t *terminal, void *stream);

/* q f32[B][4] = reward + (float)gamma * ((sum over the n_e = nchild / 2 cells j, ascending, of 0.9f * v[2j] + 0.1f * v[2j+1])
 * / n_e), v = values f32[N] of the pair's children with 0 where terminal (a select: a terminal child's value is never
 * read into the sum); every product and sum rounded to f32 on its own.  q = 0 where nchild = 0.  One lane per (b, a).
 * G2048_EINVAL: a null pointer (values / terminal may be null when N = 0), B outside 1 .. 2^24, N < 0 or N > 120 * B,
 * values not 8-byte aligned, terminal not 2-byte aligned, the others not 4-byte aligned. */
int g2048_lookahead_reduce(const float *reward, const int32_t *nchild, const int32_t *offset, const float *values,
                           const uint8_t *terminal, double gamma, int64_t B, int64_t N, float *q, void *stream);

/* ---- two-ply expectimax over the critic --------------------------------------------------------------------------------
 * V1(s') = 0 if s' is terminal, else max over the legal a' of [ r(s', a') + gamma * E_spawn V(s'') ], V(terminal s'') = 0;
 * Q2(s, a) = r(s, a) + gamma * E_spawn V1(s').  The three kernels above run on both levels (a level-1 child is a board):
 * expand(boards) -> children -> expand(children1) -> dedup -> children(after2, nuniq) -> V(children2) ->
 * reduce(reward = 0, nuniq) = e -> backup = V1 -> reduce(reward1, nchild1, values = V1) = Q2.  The level-2 pairs are indexed
 * p = 4 * c + a' over the N1 level-1 children c; the pairs of one root are contiguous (its children are). */

/* Duplicate afterstates within each root.  group_start i32[G + 1] (device): root g owns the pairs group_start[g] ..
 * group_start[g + 1], at most 480 (120 children x 4 actions), group_start[G] = P = 4 * N1.  For a pair p with nchild[p] > 0,
 * rep[p] = the smallest p' of the same group with nchild[p'] > 0 and the same 16 bytes after[p']; for nchild[p] = 0, rep[p] = p.
 * nuniq[p] = nchild[p] if rep[p] = p, else 0: the counts of the children that still need a value.  Two pairs with one
 * afterstate have the same spawn children, hence the same expectation.  One workgroup per root, the root's keys staged in LDS
 * (at most 7680 B), every lane scans the keys before its own pair; no atomics, the output does not depend on scheduling.
 * rep / nuniq i32[P]; entries at or past P are not touched.  group_start lives on the device, so a group whose bounds disagree
 * (negative, past P, more than 480 pairs) cannot be refused by the host: the kernel gives the part of its range inside 0 .. P
 * rep = p, nuniq = 0 (no child of it is valued), and a decreasing pair of bounds writes nothing.  P = 0 launches nothing.
 * G2048_EINVAL: a null pointer, G outside 1 .. 2^24, P < 0, P not a multiple of 4, P > 2^26, P > 480 * G (some group would
 * be larger than 480 pairs), after not 16-byte aligned, the others not 4-byte aligned. */
int g2048_lookahead_dedup(const uint8_t *after, const int32_t *nchild, const int32_t *group_start, int64_t G, int64_t P, int32_t *rep,
                          int32_t *nuniq, void *stream);

/* v1 f32[N1]: v1[c] = max over the a' with nchild[c][a'] > 0 of reward[c][a'] + e[rep[c][a']] (each sum rounded to f32, the
 * max exact), 0 if there is none.  e f32[4 * N1] is g2048_lookahead_reduce's output with an all-zero reward on the nuniq
 * counts: gamma * mean at representatives (0 + x is exact, so reward + e[rep] rounds as reward + gamma * mean does without
 * dedup).  One lane per level-1 child, one 16-byte load each of its rewards, counts and reps; a rep outside 0 .. 4 * N1
 * removes the action.  G2048_EINVAL: a null pointer, N1 outside 1 .. 2^24, reward / nchild / rep not 16-byte aligned, e / v1
 * not 4-byte aligned. */
int g2048_lookahead_backup(const float *reward, const int32_t *nchild, const int32_t *rep, const float *e, int64_t N1, float *v1,
                           void *stream);

/* ---- canonical frame: the dihedral symmetry of the board around the policy forward ---------------------------------------
 * (no reference counterpart: the reference's forward, src/ppo/torch_action_wrapper.py:73-102, sees the board as it lies; these
 * two kernels wrap that forward.)  A position has eight equivalent views g = 4 f + k, f in {0, 1}, k in 0 .. 3:
 * view_g(board) = np.rot90(T_f(board as 4 x 4), k) flattened row-major, T_1 the transpose, T_0 the identity.  The action that
 * does in view g what a does in the env's frame (0 left, 1 up, 2 right, 3 down) is sigma_g(a) = ((a ^ f) - k) mod 4:
 * move(view_g(s), sigma_g(a)) = view_g(move(s, a)) with the same merge score.  canon(s) is the view whose 16 bytes, compared
 * from cell 0 upward, are lexicographically largest, frame(s) the smallest g that attains it; canon(view_h(s)) = canon(s) for
 * every h.  The policy pi'(a | s) = pi_net(sigma_g(a) | canon(s)), g = frame(s), is exactly equivariant and its value
 * exactly invariant, for one forward. */

/* out_boards[b] = canon(boards[b]) (one 16-byte store), frame[b] = frame(boards[b]), out_actions[b] =
 * sigma_g(actions[b] & 3), out_masks[b]: bit sigma_g(a) = bit a of masks[b], bits 4 .. 7 zero (g = frame(boards[b])).
 * actions / out_actions and masks / out_masks are optional, null together; frame is optional on its own.  Every output may be
 * the same pointer as its input (the in-place pass over a rollout buffer); any other overlap is the caller's error.  One lane
 * per board; rows at or past B are not touched.
 * G2048_EINVAL: null boards or out_boards, exactly one pointer of an optional pair, B outside 1 .. 2^30, boards or out_boards
 * not 16-byte aligned. */
int g2048_sym_canon(const uint8_t *boards, const uint8_t *actions, const uint8_t *masks, int64_t B, uint8_t *out_boards,
                    uint8_t *out_actions, uint8_t *out_masks, uint8_t *frame, void *stream);

/* out f32[B][4]: out[b][a] = logits[b][sigma_g(a)], g = frame[b] & 7: the canonical-frame logits of the forward back in the
 * env's frame.  One 16-byte load and one 16-byte store per lane; the f32 bit patterns are moved, not recomputed (NaN payloads
 * and the sign of zero survive).  out may be logits.
 * G2048_EINVAL: a null pointer, B outside 1 .. 2^30, logits or out not 16-byte aligned. */
int g2048_sym_logits(const float *logits, const uint8_t *frame, int64_t B, float *out, void *stream);

/* Eight-view ensemble: instead of one forward in a chosen frame, one forward on all eight views and the mean over them,
 *   L(s)[a] = 1/8 sum_g net_logits(view_g(s))[sigma_g(a)],   V(s) = 1/8 sum_g net_value(view_g(s)).
 * The views of view_h(s) are the views of s in another order (view_g(view_h(s)) = view_c(s), sigma_g(sigma_h(a)) = sigma_c(a),
 * c a permutation of g for every h), so the eight addends of L(view_h(s))[sigma_h(a)] are those of L(s)[a] as a multiset.  The
 * mean is therefore taken in an order that depends on the multiset only: the addends are sorted by the total order of their
 * bit patterns (-NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN), added in ascending order, each f32 add rounded on its own,
 * and the sum is multiplied by 0.125f.  With a network whose output for a row depends on that row alone, any agent becomes
 * exactly equivariant in policy and exactly invariant in value, without retraining.  The result is NaN whenever an addend is
 * NaN or both infinities occur (payload unspecified). */

/* views u8[B][8][16]: views[b][g] = view_g(boards[b]).  One lane per output row r = 8 b + g, one 16-byte load and one 16-byte
 * store each; rows at or past 8 B are not touched.  boards is read only and may not overlap views.
 * G2048_EINVAL: a null pointer, B outside 1 .. 2^27, boards or views not 16-byte aligned. */
int g2048_sym_views(const uint8_t *boards, int64_t B, uint8_t *views, void *stream);

/* logits f32[8 B][4], values f32[8 B]: a forward's outputs on g2048_sym_views' rows.  out_logits f32[B][4]: out_logits[b][a] =
 * the mean above of the eight logits[8 b + g][sigma_g(a)]; out_values f32[B]: the same of values[8 b + g].  The pairs
 * (logits, out_logits) and (values, out_values) are each optional, null together; an output that is not asked for is not
 * written, rows at or past B are not touched.  One lane per board: 160 B read, 20 B written.  No output may overlap an input.
 * G2048_EINVAL: exactly one pointer of a pair, both pairs null, B outside 1 .. 2^27, logits or out_logits not 16-byte aligned,
 * values or out_values not 4-byte aligned. */
int g2048_sym_fold(const float *logits, const float *values, int64_t B, float *out_logits, float *out_values, void *stream);

/* ---- Monte-Carlo playouts (no reference counterpart: the reference's play only ever asks the actor) -----------------------
 * For every root board s and every action a, R playouts of a cheap policy from the afterstate:
 *   Q(s, a) = 1/R sum_r [ sum_t gamma^t r_t  + gamma^d V(leaf_r) ]      (the V term only with leaf values, only for a playout
 *                                                                         that was cut off alive; Q of an illegal a is +0)
 * A call has B roots and n = 4 B R lanes: lane j = (4 b + a) R + r is playout r of pair (b, a), and its keys are those of index
 * g = lane0 + j among n_total (keys = split(sub, n_total)[g], as env0 / B_total of the fused engine: a call cut into slices of
 * whole boards draws the keys of the uncut call).  Lane state: lane_boards u8[n][16], lane_masks u8[n], lane_done u8[n],
 * lane_ret f32[n] (discounted return so far), lane_disc f32[n] (gamma^steps played).
 *   seeding, global step 0: board = roots[b], mask = legal mask of the root, done = !(mask >> a & 1), ret = +0, disc = 1
 *   a step t of a lane with done == 0: action = a at t == 0 (the act sub-key of step 0 is not used), else the playout policy
 *     (act_randomly with key split(act_sub_t, n_total)[g], or act_drul) on the lane's mask; r = env.step with key
 *     split(step_sub_t, n_total)[g]; ret = ret + disc * r, then disc = disc * (float)gamma, every f32 operation rounded on its
 *     own.  A finished lane is frozen. */

/* n_steps steps (1 .. G2048_MAX_FUSED_STEPS) of every lane, boards resident in registers across them, no trajectory written:
 * 26 B of lane state read and written per lane (t0 == 0: the 16 B root read instead).  step_subs (host) = [n_steps][4]: act
 * sub-key, step sub-key of global steps t0 .. t0 + n_steps - 1.  t0 == 0 seeds the lanes from roots u8[B][16] and the lane
 * arrays are output only; t0 > 0 continues from the lane arrays and roots is not read (may be NULL).  Lanes at or past 4 B R are
 * not touched.  *live_count (device u32, zeroed by the caller; may be NULL) += lanes still running afterwards, one atomic per
 * workgroup that has any.
 * G2048_EINVAL: null step_subs or lane array, null roots at t0 == 0, n_steps outside 1 .. G2048_MAX_FUSED_STEPS, t0 < 0,
 * R outside 1 .. 1024, B < 1, lane0 < 0, n_total outside 1 .. 2^31 - 1, lane0 + 4 B R > n_total, policy not G2048_POLICY_DRUL /
 * G2048_POLICY_RANDOM, gamma outside (0, 1] (NaN included), unknown rng_mode, roots or lane_boards not 16-byte aligned,
 * lane_ret, lane_disc or live_count not 4-byte aligned. */
int g2048_mc_playout(const uint32_t *step_subs /*host*/, int n_steps, int64_t t0, const uint8_t *roots, int64_t B, int R,
                     int64_t lane0, int64_t n_total, int policy, double gamma, uint8_t *lane_boards, uint8_t *lane_masks,
                     uint8_t *lane_done, float *lane_ret, float *lane_disc, int rng_mode, uint32_t *live_count, void *stream);

/* q f32[B][4]: q[b][a] = (x_0 + x_1 + .. + x_{R-1}) / (float)R over the R lanes of pair (b, a), added in ascending r starting
 * from +0, each add and the one division rounded on their own.  x_r = lane_ret[r] when leaf_values is NULL or the lane is done,
 * else lane_ret[r] + lane_disc[r] * leaf_values[r] (leaf_values f32[4 B R]: the critic on lane_boards; a finished lane's value
 * is never read into the sum).  One lane per pair walks its R consecutive lanes: no atomics, the bits do not depend on
 * scheduling.  Rows at or past B are not touched.
 * G2048_EINVAL: null lane_ret, lane_disc, lane_done or q, R outside 1 .. 1024, B < 1, 4 B R >= 2^31, an f32 array not 4-byte
 * aligned. */
int g2048_mc_reduce(const float *lane_ret, const float *lane_disc, const uint8_t *lane_done, const float *leaf_values, int64_t B,
                    int R, float *q, void *stream);

/* ---- n-tuple network (no reference counterpart: a value function made of table lookups, learned by TD(0) on afterstates) ----
 * m tuples (1 .. 8) of L distinct cells each (1 .. 6, row-major cell indices 0 .. 15): tuple_cells u8[m][L], a HOST pointer
 * whose bytes travel in the kernarg.  weights i32[m][16^L], fixed point with frac_bits F (0 .. 20) fractional bits.
 *   idx(x, t) = sum_j min(x[c_tj], 15) << 4 j             (log2 tiles above 15 are clamped: the index never leaves the table)
 *   S(board)  = sum over g = 0 .. 7 and t of weights[t][idx(view_g(board), t)], an int64 sum; view_g as in the canonical frame
 *   V(board)  = (float)S * 2^-F: one int64 -> f32 conversion (round to nearest even), one exact multiply
 * Batch-synchronous TD(0): every env keeps prev_after u8[16], the afterstate of its last move, and flag u8: 0 no predecessor,
 * 1 a predecessor whose successor is the env's current board, 2 a predecessor whose step ended the episode.  Per lock-step,
 * with target = v(current board) for flag 1 and 0 for flag 2:
 *   e = target - V(prev_after) (one f32 subtraction), d = e * c with c = (float)(alpha * 2^F / (8 m)) (computed in double),
 *   d clamped to +-2^30, delta = (int32) rint(d) (half to even);
 *   accumulate: for every env with flag != 0, every view g and tuple t: acc[t][i] += delta, cnt[t][i] += 1 at
 *     i = idx(view_g(prev_after), t); a board that hits an entry several times counts each time;
 *   apply: for every entry with cnt > 0: weights = sat_int32(weights + rdiv(acc, cnt)), acc = cnt = 0, with
 *     rdiv(a, c) = sign(a) * ((2 |a| + c) / (2 c)) in int64 (the mean, rounded half away from zero).
 * acc i64[m][16^L] and cnt i32[m][16^L] are all-zero between lock-steps.  Every accumulation is an integer one: the result
 * does not depend on scheduling.  No entry point allocates or synchronises; every argument check precedes any device work. */

/* values f32[n]: values[i] = V(boards[i]).  One lane per board, 8 m gathers each; rows at or past n are not touched.
 * G2048_EINVAL: a null pointer, n outside 1 .. 2^28, m outside 1 .. 8, L outside 1 .. 6, a cell above 15, a cell twice in one
 * tuple, frac_bits outside 0 .. 20, boards not 16-byte aligned, weights or values not 4-byte aligned. */
int g2048_ntuple_values(const uint8_t *boards, int64_t n, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m, int L,
                        int frac_bits, float *values, void *stream);

/* scores f32[B][4]: scores[b][a] = (float)r_a + V(after_a) (one rounded add) with after_a, r_a = move(boards[b], a) where
 * after_a != boards[b], +0 where the move is illegal.  values f32[B]: the max of scores[b] over the legal a, 0 if there is
 * none.  One lane per (board, action) pair, all 8 m gathers of a lane in flight together, the max by quad cross-lane moves;
 * rows at or past B are not touched.
 * G2048_EINVAL: as g2048_ntuple_values (B for n), scores not 4-byte aligned. */
int g2048_ntuple_scores(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m, int L,
                        int frac_bits, float *scores, float *values, void *stream);

/* The accumulate half of a lock-step (above).  prev_after u8[B][16], flag u8[B], target f32[B] (read where flag == 1 only);
 * weights are only read.  td_error f32[B] (may be NULL) = e, 0 where flag == 0.  One lane per env: 8 m gathers, then 8 m
 * 64-bit and 8 m 32-bit atomic adds.
 * G2048_EINVAL: a null pointer other than td_error, B outside 1 .. 2^28, the network as above, alpha not a finite positive
 * number, prev_after not 16-byte aligned, acc not 8-byte aligned, target, weights, cnt or td_error not 4-byte aligned. */
int g2048_ntuple_td_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B,
                               const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m, int L, int frac_bits, double alpha,
                               int64_t *acc, int32_t *cnt, float *td_error, void *stream);

/* The apply half, in a launch of its own after g2048_ntuple_td_accumulate on the same prev_after and flag: the entries of the
 * same boards are visited again, cnt is exchanged for 0 and the one lane that finds cnt > 0 updates the entry.  The tables
 * are never scanned: the cost is that of the 8 m entries per env.
 * G2048_EINVAL: a null pointer, B outside 1 .. 2^28, the network as above, prev_after not 16-byte aligned, acc not 8-byte
 * aligned, weights or cnt not 4-byte aligned. */
int g2048_ntuple_td_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells /*host*/, int m, int L,
                          int32_t *weights, int64_t *acc, int32_t *cnt, void *stream);

/* After the env step: prev_after[b] = move(tr_boards_row[b], action), flag[b] = done_after ? 2 : 1, action and done_after read
 * from tr_meta_row[b] = action | mask_before << 2 | done_after << 6, the trajectory row the engine has just written (the
 * learner follows whatever the policy played).  One lane per env.
 * G2048_EINVAL: a null pointer, B outside 1 .. 2^28, tr_boards_row or prev_after not 16-byte aligned. */
int g2048_ntuple_link(const uint8_t *tr_boards_row, const uint8_t *tr_meta_row, int64_t B, uint8_t *prev_after, uint8_t *flag,
                      void *stream);

/* ---- n-tuple expectimax (one or two plies of search over the n-tuple network, inside the kernel) ----
 * All f32, every operation individually rounded, table sums integer as above; order and rounding as g2048_lookahead_reduce.
 *   Q0(s,a), V0(s) = scores and values of g2048_ntuple_scores
 *   for k = 1, 2:
 *     acc      = sum over the empty cells c of after_a(s), ascending cell index, starting from +0, of
 *                0.9f * V_{k-1}(after_a + tile 2 at c) + 0.1f * V_{k-1}(after_a + tile 4 at c)
 *     Q_k(s,a) = (float)r(s,a) + gamma * (acc / (float)n_empty) where a is legal (correctly rounded division), +0 where not
 *     V_k(s)   = the max of Q_k(s,a) over the legal a, +0 if there is none (so a child without a legal move is worth +0)
 * The children of a board have fixed slots, slot = a * 32 + cell * 2 + (tile - 1) (128 of them; a slot exists if a is legal and
 * the cell is empty in after_a): nothing is enumerated, counted or scanned, no child board reaches memory, nothing is read
 * back.  One ply is one launch of one workgroup per root; two plies are one workgroup per (root, slot) that writes V1 of the
 * child to workspace[root * 128 + slot], then one lane per (root, action).  A workspace entry whose slot does not exist is
 * neither written nor read: the workspace needs no clearing and its contents do not change the result.  No atomics: the bits
 * do not depend on scheduling. */

/* The f32 elements of workspace that g2048_ntuple_expectimax needs: 0 for plies == 1, 128 B for plies == 2; -1 for plies not 1
 * or 2, B < 1, B > 2^24 (one ply) or B > 2^20 (two plies). */
int64_t g2048_ntuple_expectimax_workspace_floats(int64_t B, int plies);

/* scores f32[B][4] = Q_plies(boards[b], a), values f32[B] = V_plies(boards[b]); rows at or past B are not touched.  gamma is
 * rounded to f32 once.
 * G2048_EINVAL, before any device work: a null pointer (workspace may be null when plies == 1), B or plies for which
 * g2048_ntuple_expectimax_workspace_floats returns -1, the network or frac_bits as for g2048_ntuple_values, gamma negative or
 * not finite, boards not 16-byte aligned, weights, scores or values not 4-byte aligned, workspace not 8-byte aligned. */
int g2048_ntuple_expectimax(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m,
                            int L, int frac_bits, int plies, double gamma, float *workspace, float *scores, float *values,
                            void *stream);

/* ---- n-tuple TC learning (temporal coherence: every table entry has its own step size, all of it integer arithmetic) ----
 * A second learner for the n-tuple network above, in place of the td_accumulate / td_apply pair of a lock-step.  prev_after,
 * flag, target, e, c and delta are exactly those of TD(0).  Two more tables next to weights, coh_e i32[m][16^L] and coh_a
 * i32[m][16^L] (E and A below, all-zero at the start: rate 1), and one more accumulator, abs_acc i64[m][16^L]:
 *   accumulate: for every env with flag != 0, every view g and tuple t: acc += delta, abs_acc += |delta|, cnt += 1;
 *   apply: for every entry with n = cnt > 0:
 *     d = rdiv(acc, n), a = rdiv(abs_acc, n)                      (a >= |d| because |acc| <= abs_acc)
 *     step = A == 0 ? d : rdiv(d * |E|, A)                        (the rate |E| / A is read before the entry's own update;
 *                                                                  |d| <= 2^30 and |E| <= A < 2^31: the product is < 2^61)
 *     weights = sat_int32(weights + step);  E += d;  A += a       (in int64)
 *     if A >= 2^31: E = sign(E) * (|E| / 2), A = A >> 1           (once suffices, A < 2^31 + 2^30; keeps |E| <= A < 2^31)
 *     acc = abs_acc = cnt = 0.
 * From all-zero coh_e and coh_a one lock-step moves the weights exactly as TD(0) does.  acc, abs_acc and cnt are all-zero
 * between lock-steps.  Every accumulation is an integer one: the result does not depend on scheduling. */

/* The accumulate half.  Operands as g2048_ntuple_td_accumulate plus abs_acc; weights are only read.  td_error f32[B] (may be
 * NULL) = e, 0 where flag == 0.  One lane per env: 8 m gathers, then 16 m 64-bit and 8 m 32-bit atomic adds.
 * G2048_EINVAL: a null pointer other than td_error, B outside 1 .. 2^28, the network or frac_bits as for g2048_ntuple_values,
 * alpha not a finite positive number, prev_after not 16-byte aligned, acc or abs_acc not 8-byte aligned, target, weights, cnt
 * or td_error not 4-byte aligned. */
int g2048_ntuple_tc_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B,
                               const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m, int L, int frac_bits, double alpha,
                               int64_t *acc, int64_t *abs_acc, int32_t *cnt, float *td_error, void *stream);

/* The apply half, in a launch of its own after g2048_ntuple_tc_accumulate on the same prev_after and flag: cnt is exchanged for
 * 0 at the entries of the same boards and the one lane that finds cnt > 0 updates weights, coh_e, coh_a and clears acc and
 * abs_acc there.  The tables are never scanned.
 * G2048_EINVAL: a null pointer, B outside 1 .. 2^28, the network as above, prev_after not 16-byte aligned, acc or abs_acc not
 * 8-byte aligned, weights, cnt, coh_e or coh_a not 4-byte aligned. */
int g2048_ntuple_tc_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells /*host*/, int m, int L,
                          int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a,
                          void *stream);

/* ---- multi-stage n-tuple network (one set of tables per max-tile stage of the game) ----
 * stage_tiles u8[n_stages - 1], a HOST pointer whose bytes travel in the kernarg: log2 tile values k_1 < k_2 < ... in 1 .. 17.
 * n_stages S is 1 .. 8.  Every table of the network above (weights, acc, cnt, abs_acc, coh_e, coh_a) becomes [S][m][16^L], and
 *   stage(x)     = #{ i : max over the 16 cells of x[c] >= k_i }   (the UNCLAMPED log2 tile: 16 and 17 count as themselves)
 *   off(x, g, t) = ((stage(x) * m + t) << 4 L) + idx(view_g(x), t)  (idx as above, with its clamp)
 * takes the place of t 16^L + idx in S(x); V, scores, the expectimax recursion, e, delta, acc / cnt / abs_acc / coh_e / coh_a and
 * rdiv are exactly those above.  The stage is that of the board that is looked up: in scores the AFTERSTATE (a merge that
 * creates tile k_i is valued by stage i's tables), in expectimax each leaf's afterstate, in the learners prev_after.  The
 * maximum is the same in all eight views, so it is taken once per board.  S <= 8, m <= 8 and L <= 6 keep an offset below 2^30.
 * The kernels know nothing of promotion: a caller whose upper stages are not split off yet passes the first p - 1 thresholds
 * and n_stages = p, and boards at or above k_p are then served and learned by stage p - 1's tables.
 * Each function has the unstaged signature with (stage_tiles, n_stages) after L, and the unstaged function IS the staged one
 * called with (NULL, 1): one kernel per operation.  n_stages == 1 accepts a null stage_tiles (it is not read).
 * G2048_EINVAL, before any device work, on top of every check of the unstaged function: n_stages outside 1 .. 8, a null
 * stage_tiles with n_stages > 1, a threshold outside 1 .. 17, thresholds not strictly ascending.  g2048_ntuple_link and
 * g2048_ntuple_expectimax_workspace_floats do not depend on the stages. */
int g2048_ntuple_staged_values(const uint8_t *boards, int64_t n, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m,
                               int L, const uint8_t *stage_tiles /*host*/, int n_stages, int frac_bits, float *values, void *stream);
int g2048_ntuple_staged_scores(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m,
                               int L, const uint8_t *stage_tiles /*host*/, int n_stages, int frac_bits, float *scores, float *values,
                               void *stream);
int g2048_ntuple_staged_expectimax(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/,
                                   int m, int L, const uint8_t *stage_tiles /*host*/, int n_stages, int frac_bits, int plies,
                                   double gamma, float *workspace, float *scores, float *values, void *stream);
int g2048_ntuple_staged_td_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B,
                                      const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m, int L,
                                      const uint8_t *stage_tiles /*host*/, int n_stages, int frac_bits, double alpha, int64_t *acc,
                                      int32_t *cnt, float *td_error, void *stream);
int g2048_ntuple_staged_td_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells /*host*/, int m,
                                 int L, const uint8_t *stage_tiles /*host*/, int n_stages, int32_t *weights, int64_t *acc,
                                 int32_t *cnt, void *stream);
int g2048_ntuple_staged_tc_accumulate(const uint8_t *prev_after, const uint8_t *flag, const float *target, int64_t B,
                                      const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m, int L,
                                      const uint8_t *stage_tiles /*host*/, int n_stages, int frac_bits, double alpha, int64_t *acc,
                                      int64_t *abs_acc, int32_t *cnt, float *td_error, void *stream);
int g2048_ntuple_staged_tc_apply(const uint8_t *prev_after, const uint8_t *flag, int64_t B, const uint8_t *tuple_cells /*host*/, int m,
                                 int L, const uint8_t *stage_tiles /*host*/, int n_stages, int32_t *weights, int64_t *acc,
                                 int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a, void *stream);

/* ---- n-tuple frontier search (1 .. 3 plies of expectimax over the n-tuple network on packed, deduplicated lists of afterstates) ----
 * A second path next to g2048_ntuple_expectimax, with the same arithmetic continued one level.  For an afterstate x with n >= 1
 * empty cells and j >= 1:
 *   E_j(x)   = acc / (float)n (correctly rounded), acc = sum over the empty cells c of x, ascending, starting from +0, of
 *              0.9f * V_{j-1}(x + tile 2 at c) + 0.1f * V_{j-1}(x + tile 4 at c)
 *   V_0(p)   = values of g2048_ntuple_scores
 *   V_j(p)   = the max over the legal a of (float)r(p,a) + gamma * E_j(after_a(p)), +0 if there is none
 *   Q_d(s,a) = (float)r(s,a) + gamma * E_d(after_a(s)) where a is legal, +0 where not
 * Every f32 operation is individually rounded; at depth 1 and 2 scores and values equal g2048_ntuple_expectimax's bit for bit.
 * The frontier of level j is a list of afterstates: A_1 holds the legal afterstates of the roots, A_{j+1} the afterstates
 * after_a'(x + tile at c) over the entries x of A_j, their empty cells, both tiles and the legal a'.  Per root, without merging,
 * |A_1| <= 4, |A_2| <= 480, |A_3| <= 57 600.  With dedup != 0 two entries of one level that descend from the same root and hold the
 * same 16 bytes are one entry; E_j is a function of the board alone, so merging changes no output bit.  Equality is decided on the
 * 16 bytes.  Merging is complete while a root's level has at most 8 192 unique entries; past that, entries may be appended unmerged
 * (same bits, more entries).  Roots are never merged with each other.  The lists, the links between the levels and E_j live in
 * the caller's workspace, sized for the worst case so that no list can overflow; its contents before the call do not matter.
 * List space is taken from one device-side counter per level: the order of a list depends on scheduling, no value does. */

/* The bytes of workspace for B roots at `depth`: about 0.1 KB per root at depth 1, 12 KB at depth 2, 1.41 MB at depth 3.  -1 for a
 * depth outside 1 .. 3, B < 1, or B above 2^20 (depth 1), 2^16 (depth 2), 2^12 (depth 3). */
int64_t g2048_ntuple_search_workspace_bytes(int64_t B, int depth);

/* scores f32[B][4] = Q_depth(boards[b], a), values f32[B] = V_depth(boards[b]); rows at or past B and workspace bytes at or past
 * g2048_ntuple_search_workspace_bytes(B, depth) are not touched.  counts i32[3] (device, may be NULL) = |A_1|, |A_2|, |A_3| as
 * built, 0 for the levels beyond depth.  gamma is rounded to f32 once.
 * G2048_EINVAL, before any device work: a null pointer other than counts, B or depth for which
 * g2048_ntuple_search_workspace_bytes returns -1, workspace_bytes below that size, the network or frac_bits as for
 * g2048_ntuple_values, gamma negative or not finite, boards or workspace not 16-byte aligned, weights, scores, values or counts
 * not 4-byte aligned. */
int g2048_ntuple_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m, int L,
                        int frac_bits, int depth, double gamma, int dedup, void *workspace, int64_t workspace_bytes, float *scores,
                        float *values, int32_t *counts, void *stream);

/* The same over a multi-stage network (stage_tiles, n_stages as above): every leaf is looked up in its own stage. */
int g2048_ntuple_staged_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m,
                               int L, const uint8_t *stage_tiles /*host*/, int n_stages, int frac_bits, int depth, double gamma,
                               int dedup, void *workspace, int64_t workspace_bytes, float *scores, float *values, int32_t *counts,
                               void *stream);

/* ---- n-tuple budgeted search (the frontier search, every root as deep as its levels stay within a budget of unique entries) ----
 * A third path next to g2048_ntuple_expectimax and g2048_ntuple_search.  With A_j, E_j, V_j and Q_d exactly as above, the order of
 * every f32 operation included, and merging always on:
 *   U_j(s) = the number of distinct 16-byte afterstates in A_j(s)
 *   d(s)   = the largest d in 1 .. max_depth with U_j(s) <= budget for every j <= d
 *   scores(s, a) = Q_{d(s)}(s, a),   values(s) = the max over the legal a, +0 if there is none
 * U_1 <= 4 <= budget, so d >= 1.  A root without a legal move has U_j = 0 everywhere: it reports d = max_depth and all-zero scores.
 * U_j is a function of the root's 16 bytes alone, so d(s) and every output bit are the same in every run.  A root's result equals
 * g2048_ntuple_search at depth d(s) bit for bit wherever that exists (d <= 3), and g2048_ntuple_expectimax at d <= 2.  A level that
 * would outgrow the budget is abandoned while it is built and never evaluated.  Every root owns a fixed region per level of the
 * caller's workspace: 4 entries at level 1, 480 at level 2, budget + 512 from level 3 on; its contents before the call do not matter. */

/* The bytes of workspace for B roots.  Per root: 532 bytes per entry of every level's region but the last (list, E, 128 links), 20
 * per entry of the last; about 5.1 MB at max_depth 4, budget 8 192 and 27.5 MB at max_depth 5, budget 24 576.  -1 for max_depth
 * outside 1 .. 6, budget outside 4 .. 24 576, B < 1, or B above the per-call limit min(2^20, floor((2^31 - 1) / (128 * the entries
 * of the largest region))): 668 at budget 24 576 and 1 927 at budget 8 192 from max_depth 3 on, 34 952 at max_depth 2, 2^20 at
 * max_depth 1.  Within it every element index stays below 2^31 and the workspace below 2^36 bytes. */
int64_t g2048_ntuple_budget_search_workspace_bytes(int64_t B, int max_depth, int budget);

/* scores f32[B][4], values f32[B] as defined above; depth_used u8[B] (device, may be NULL) = d(s); entries i32[B][6] (device, may be
 * NULL) = U_j for j <= d(s), 0 beyond.  Rows at or past B and workspace bytes at or past
 * g2048_ntuple_budget_search_workspace_bytes(B, max_depth, budget) are not touched.  gamma is rounded to f32 once.
 * G2048_EINVAL, before any device work: everything g2048_ntuple_search refuses (a null pointer other than depth_used and entries,
 * workspace_bytes below the size, the network, frac_bits, gamma negative or not finite, boards or workspace not 16-byte aligned,
 * weights, scores, values or entries not 4-byte aligned), and a B, max_depth or budget for which the size function returns -1. */
int g2048_ntuple_budget_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/, int m,
                               int L, int frac_bits, int max_depth, int budget, double gamma, void *workspace, int64_t workspace_bytes,
                               float *scores, float *values, uint8_t *depth_used, int32_t *entries, void *stream);

/* The same over a multi-stage network (stage_tiles, n_stages as above): every leaf is looked up in its own stage. */
int g2048_ntuple_staged_budget_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells /*host*/,
                                      int m, int L, const uint8_t *stage_tiles /*host*/, int n_stages, int frac_bits, int max_depth,
                                      int budget, double gamma, void *workspace, int64_t workspace_bytes, float *scores, float *values,
                                      uint8_t *depth_used, int32_t *entries, void *stream);

/* ---- n-tuple carousel (carousel shaping: episode starts from per-stage pools of boards, so every stage is trained) ----
 * For a trainer over B always-live envs, after the auto-reset env step and g2048_ntuple_link of a lock-step.  The carousel has its
 * own thresholds carousel_tiles u8[n_tiles], a HOST pointer whose bytes travel in the kernarg: log2 tile values k_1 < ... < k_n in
 * 1 .. 17, n in 1 .. 7, all always in use, and
 *   cs(x) = #{ i : max over the 16 cells of x[c] >= k_i }            (the UNCLAMPED log2 tile: stage(x) above over these thresholds)
 * State, all-zero at the start: pool_boards u8[n][B][16] and pool_masks u8[n][B] (slot (i, b) belongs to env b and is empty exactly
 * when its mask is 0), reached u8[B] (the highest carousel stage env b's episode has recorded), turn u32[B], starts i64[n + 1].
 * flag is g2048_ntuple_link's: 1 the episode goes on, 2 the step ended it and boards / masks hold the engine's fresh board.
 *   record:  for every env b with flag == 1 and s = cs(boards[b]) > reached[b]: pool_boards[s-1][b] = boards[b],
 *            pool_masks[s-1][b] = masks[b] (as it is, also 0), reached[b] = s.  Only slot s - 1, also when s jumps by several.
 *   restart: for every env b with flag == 2: turn[b] += 1 (u32 wrap), c = (u32)(b + turn[b]) % (n + 1).  If c >= 1:
 *            j = bits(split(sub, B)[b]) % B (32 bits, shape ()), and if pool_masks[c-1][j] != 0: boards[b] = pool_boards[c-1][j],
 *            masks[b] = pool_masks[c-1][j], reached[b] = c, starts[c] += 1, start_stage[b] = c.  In every other case the fresh
 *            board stays, reached[b] = 0, starts[0] += 1, start_stage[b] = 0.  An env with flag != 2: start_stage[b] = 0xFF only.
 * record writes only the env's own slots and restart writes no slot: neither launch races with itself.  restart reads what the
 * same lock-step's record wrote, so they are two launches.  All of it is integer arithmetic; starts is updated by 64-bit atomic
 * adds, so nothing depends on scheduling. */

/* The record half.  boards u8[B][16] / masks u8[B]: the envs' state for the next step.  One lane per env.
 * G2048_EINVAL, before any device work: a null pointer, B outside 1 .. 2^28, n_tiles outside 1 .. 7, a threshold outside 1 .. 17,
 * thresholds not strictly ascending, boards or pool_boards not 16-byte aligned. */
int g2048_ntuple_carousel_record(const uint8_t *boards, const uint8_t *masks, const uint8_t *flag, int64_t B,
                                 const uint8_t *carousel_tiles /*host*/, int n_tiles, uint8_t *reached,
                                 uint8_t *pool_boards, uint8_t *pool_masks, void *stream);

/* The restart half, in a launch of its own after g2048_ntuple_carousel_record.  (sub0, sub1): the lock-step's act sub-key, from
 * which a greedy step (sample == 0) draws nothing.  start_stage u8[B] may be NULL.  One lane per env.
 * G2048_EINVAL, before any device work: a null pointer other than start_stage, B outside 1 .. 2^28, n_tiles outside 1 .. 7, an
 * unknown rng_mode, boards or pool_boards not 16-byte aligned, turn not 4-byte aligned, starts not 8-byte aligned. */
int g2048_ntuple_carousel_restart(uint32_t sub0, uint32_t sub1, const uint8_t *flag, int64_t B, int n_tiles,
                                  const uint8_t *pool_boards, const uint8_t *pool_masks, uint8_t *boards, uint8_t *masks,
                                  uint8_t *reached, uint32_t *turn, int64_t *starts, uint8_t *start_stage /*may be NULL*/,
                                  int rng_mode, void *stream);

/* ---- n-tuple delayed TD(lambda) (multi-step credit: an afterstate is updated once, h - 1 lock-steps late, by a lambda-sum) ----
 * A third form of the learner's middle pair and of link, for TD(0) and TC alike (Jaskowski 2017, "delayed" TD(lambda) / TC(lambda):
 * no eligibility traces, every state is still updated exactly once).  Per trainer: the horizon h in 1 .. 8, lam in [0, 1] (a
 * double, used as its f32 value) and B envs.  Env state on top of prev_after and flag, all-zero at the start:
 *   hist u8[h][B][16], a ring of afterstates;  hist_err f32[h][B], their TD errors;  hist_len u8[B], the states the env holds.
 * The ring position is GLOBAL, not per env.  At lock-step n (the caller's count of lock-steps so far):
 *   head = (n - 1) mod h holds the newest afterstate A_{n-1}; the state j steps back (j = 1 .. hist_len) sits in slot
 *   (head - j + 1) mod h; link writes A_n to slot n mod h.
 * accumulate, for every env with flag != 0 (flag, target, V, c and the tables as for TD(0) / TC above):
 *   e = sub_rn(flag == 1 ? target : 0, V(hist[head][b])), TD(0)'s e; stored to td_error[b] and to hist_err[head][b];
 *   x_1 = hist_err[head][b], x_{j+1} = add_rn(hist_err[(head - j) mod h][b], mul_rn(lam, x_j)) for j + 1 <= hist_len[b]: the
 *     lambda-sums truncated at the ring, from the newest error back, every operation individually rounded;
 *   state j is DUE if flag == 2 (the episode ended: every j in 1 .. hist_len is flushed) or, with flag == 1, if j == h (which
 *     needs hist_len == h);
 *   every due state: delta_j = (int32) rint(clamp(mul_rn(x_j, c), +-2^30)), and at each of the 8 m entries of the board in slot
 *     (head - j + 1) mod h: acc += delta_j, cnt += 1, for TC also abs_acc += |delta_j|.  The stage is that of the UPDATED board.
 * apply takes the same due set from flag, hist_len and head; per due board it is td_apply (or, with the TC tables, tc_apply).  A
 *   second hit of one entry by the same lane finds the exchanged count 0.
 * link is g2048_ntuple_link, reads the old flag[b] before it writes the new one, stores the afterstate to prev_after[b] AND to
 *   hist[slot][b], and sets hist_len[b] = min((old flag == 2 ? 0 : hist_len[b]) + 1, h).
 * h = 1 is TD(0) / TC bit for bit, whatever lam is.  lam = 0 with h > 1 is TD(0) applied h - 1 steps late.  The last h states of an
 * episode are flushed at its end with the shorter sums they have.  A hist_len above h is read as h.  acc, abs_acc and cnt are
 * all-zero between lock-steps; everything after e is integer: the result does not depend on scheduling.
 * stage_tiles / n_stages as in the staged entry points: (NULL, 1) is the unstaged network. */

/* The accumulate half.  abs_acc null: TD(0)'s tables; non-null: TC's.  td_error f32[B] (may be NULL) = e, 0 where flag == 0.  One
 * lane per env: 8 m gathers, the lambda-sums, then per due state a 16-byte load and the atomic adds of td_accumulate / tc_accumulate.
 * G2048_EINVAL, before any device work: a null pointer other than abs_acc and td_error, B outside 1 .. 2^28, h outside 1 .. 8, head
 * outside 0 .. h - 1, lam outside [0, 1] or not finite, the network, stages, frac_bits and alpha as for
 * g2048_ntuple_staged_td_accumulate, hist not 16-byte aligned, acc or abs_acc not 8-byte aligned, hist_err, target, weights, cnt or
 * td_error not 4-byte aligned. */
int g2048_ntuple_delayed_accumulate(const uint8_t *hist, float *hist_err, const uint8_t *hist_len, const uint8_t *flag,
                                    const float *target, int64_t B, int h, int head, double lam, const int32_t *weights,
                                    const uint8_t *tuple_cells /*host*/, int m, int L, const uint8_t *stage_tiles /*host*/,
                                    int n_stages, int frac_bits, double alpha, int64_t *acc, int64_t *abs_acc /*null: TD*/,
                                    int32_t *cnt, float *td_error, void *stream);

/* The apply half, in a launch of its own after g2048_ntuple_delayed_accumulate on the same ring, flag and head.  abs_acc, coh_e and
 * coh_a all null: td_apply per due board; none null: tc_apply.
 * G2048_EINVAL, before any device work: a null pointer other than those three, some but not all of the three null, B, h, head, the
 * network and stages as above, hist not 16-byte aligned, acc or abs_acc not 8-byte aligned, weights, cnt, coh_e or coh_a not 4-byte
 * aligned. */
int g2048_ntuple_delayed_apply(const uint8_t *hist, const uint8_t *hist_len, const uint8_t *flag, int64_t B, int h, int head,
                               const uint8_t *tuple_cells /*host*/, int m, int L, const uint8_t *stage_tiles /*host*/, int n_stages,
                               int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a,
                               void *stream);

/* After the env step, in place of g2048_ntuple_link: slot = n mod h for the lock-step n that has just been played.  One lane per env.
 * G2048_EINVAL, before any device work: a null pointer, B outside 1 .. 2^28, h outside 1 .. 8, slot outside 0 .. h - 1,
 * tr_boards_row, prev_after or hist not 16-byte aligned. */
int g2048_ntuple_delayed_link(const uint8_t *tr_boards_row, const uint8_t *tr_meta_row, int64_t B, int h, int slot,
                              uint8_t *prev_after, uint8_t *flag, uint8_t *hist, uint8_t *hist_len, void *stream);

/* ---- n-tuple episodes (a whole greedy evaluation of the n-tuple network: every game to its end inside a persistent kernel) ----
 * An evaluation is N games in batches of bs: game i is env g = i mod bs of batch j = i / bs, whose size is B_total = min(bs, N - j bs)
 * (the last batch may be short).  Every game carries the head of its batch's key chain, chain u32[N][2]; the caller seeds all
 * games of batch j with the same key.  A game does what the engine does to env g of a lock-step batch of B_total under
 * g2048_ntuple_scores and g2048_policy_step(use_mask = 1, sample = 0):
 *   start: key, sub = split(key) (g2048_chain_keys); board, mask = env.init(split(sub, B_total)[g]); done = 0, ep_len = 0, score = 0
 *   a step of a game with done == 0: key, act_sub = split(key) (not used: nothing is sampled); key, step_sub = split(key);
 *     q[a] = scores of g2048_ntuple_scores on the board; l[a] = max(q[a] - (mask >> a & 1 ? 0 : 1e8f), -FLT_MAX) (one rounded
 *     subtraction), action = the first maximum of l; r = env.step(action) with key split(step_sub, B_total)[g];
 *     ep_len += 1, score += (int64) r (r is -1 for an illegal move, else the merge score: an exact integer).
 * The mask is the env's, not the "after != board" of the scores: a network whose legal scores lie below -1e8 plays an illegal
 * move exactly as the engine then does.  A finished game is frozen: board, mask, ep_len, score and chain keep what they held
 * after its terminal step.  State: boards u8[N][16], masks u8[N], done u8[N], ep_len i32[N], score i64[N], chain u32[N][2]. */

/* n_steps steps (1 .. 65 536) of every game, one quad of lanes per game, the board resident in registers across them; a wave
 * leaves early once all of its games are done.  start != 0 seeds the games from chain (the state arrays are output only);
 * start == 0 continues from the state arrays.  Either way all six arrays hold the games' state afterwards; weights are only
 * read.  Rows at or past N are not touched.  *live_count (device u32, zeroed by the caller; may be NULL) += games still running
 * afterwards, one atomic per workgroup that has any.  No host key table, no cross-workgroup communication, nothing read back.
 * G2048_EINVAL, before any device work: a null pointer other than live_count, N outside 1 .. 2^24, bs outside 1 .. 2^20, n_steps
 * outside 1 .. 65 536, the network or frac_bits as for g2048_ntuple_values, unknown rng_mode, boards not 16-byte aligned, score not
 * 8-byte aligned, chain, ep_len, weights or live_count not 4-byte aligned. */
int g2048_ntuple_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights, const uint8_t *tuple_cells /*host*/,
                          int m, int L, int frac_bits, uint32_t *chain, uint8_t *boards, uint8_t *masks, uint8_t *done,
                          int32_t *ep_len, int64_t *score, int rng_mode, uint32_t *live_count, void *stream);

/* The same over a multi-stage network (stage_tiles, n_stages as above): every afterstate is looked up in its own stage. */
int g2048_ntuple_staged_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights,
                                 const uint8_t *tuple_cells /*host*/, int m, int L, const uint8_t *stage_tiles /*host*/, int n_stages,
                                 int frac_bits, uint32_t *chain, uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len,
                                 int64_t *score, int rng_mode, uint32_t *live_count, void *stream);

/* ---- n-tuple searched episodes (a whole one-ply expectimax evaluation of the n-tuple network inside a persistent kernel) ----
 * Everything of "n-tuple episodes" above holds unchanged: the placement of game i, the seed key per batch, the chain steps per move
 * (the act sub-key consumed and unused), env.step, the frozen finished game and the six state arrays.  The one difference is the
 * move choice:
 *   q[a] = Q_1(board, a) of "n-tuple expectimax" at this gamma; l[a] = max(q[a] - (mask >> a & 1 ? 0 : 1e8f), -FLT_MAX) under the
 *   game's own mask; action = the first maximum of l.
 * So game g of batch j is env g of a lock-step batch under g2048_ntuple_expectimax(plies = 1) and g2048_policy_step(use_mask = 1,
 * sample = 0), bit for bit. */

/* n_steps steps (1 .. 65 536) of every game, one wavefront per game in one-wave workgroups, the game replicated in the wave's
 * lanes: the existing children of the board (at most 120) are packed into a list, four lanes score a child, four lanes reduce
 * the four actions.  start, the state arrays, rows at or past N and weights as for g2048_ntuple_episodes; a state written with
 * start continues under the same entry point cut into any launch sizes.  *live_count (device u32, zeroed by the caller; may be
 * NULL) += games still running afterwards, one atomic per such game and launch.  gamma is used as the f32 it is.
 * G2048_EINVAL, before any device work: everything g2048_ntuple_episodes refuses, plies other than 1, gamma negative or not finite. */
int g2048_ntuple_search_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights,
                                 const uint8_t *tuple_cells /*host*/, int m, int L, int frac_bits, int plies, float gamma,
                                 uint32_t *chain, uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score,
                                 int rng_mode, uint32_t *live_count, void *stream);

/* The same over a multi-stage network (stage_tiles, n_stages as above): every leaf's afterstate is looked up in its own stage. */
int g2048_ntuple_staged_search_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *weights,
                                        const uint8_t *tuple_cells /*host*/, int m, int L, const uint8_t *stage_tiles /*host*/,
                                        int n_stages, int frac_bits, int plies, float gamma, uint32_t *chain, uint8_t *boards,
                                        uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score, int rng_mode,
                                        uint32_t *live_count, void *stream);

/* ---- policy network (update): attention for 17-token sequences ------------------------------------- */

/* softmax(q k^T * scale) v with attention dropout, head_dim 32, Sk = 17 keys, Sq = 17 queries (or 1: the CLS row
 * of the last layer); replaces F.scaled_dot_product_attention inside the encoder layers of the update
 * (reference: nn.TransformerEncoderLayer built at src/ppo/transformer_encoder.py:138-148).
 * q/k/v (and dq/dk/dv) are bf16 with element strides (batch, token) and heads contiguous inside a token, so they may
 * point into the packed in_proj output [B][S][3][H][32] and its gradient; o/dout bf16 [B][Sq][H][32]; lse f32
 * [B][H][Sq].  The dropout mask is a function of (seed, *seed_state, element index): pass the same pair to the
 * backward.  seed_state: NULL, or a device-resident 64-bit word read by the kernel at run time, so that a launch
 * captured in a hipGraph draws a new mask on every replay once the owner advances the word between replays. */
int g2048_attn_fwd(const void *q, const void *k, const void *v, void *o, float *lse, int64_t B, int H, int Sq,
                   int64_t q_sb, int64_t q_ss, int64_t k_sb, int64_t k_ss, int64_t v_sb, int64_t v_ss, float scale,
                   float p_drop, uint64_t seed, const uint64_t *seed_state, void *stream);
int g2048_attn_bwd(const void *q, const void *k, const void *v, const void *dout, const float *lse, void *dq, void *dk,
                   void *dv, int64_t B, int H, int Sq, int64_t q_sb, int64_t q_ss, int64_t k_sb, int64_t k_ss,
                   int64_t v_sb, int64_t v_ss, float scale, float p_drop, uint64_t seed, const uint64_t *seed_state,
                   void *stream);

/* ---- policy network (update): residual add + dropout + LayerNorm, d_model 256 ------------------------ */

/* x_new = x + dropout(a);  h = bf16(LayerNorm(x_new) * gamma + beta): the tail of one pre-norm sub-layer fused with
 * the head of the next (reference: nn.TransformerEncoderLayer(norm_first=True), src/ppo/transformer_encoder.py:138-148;
 * `x = x + dropout1(sa(norm1(x)))`, `x = x + dropout2(ff(norm2(x)))`).
 * x f32 rows of 256 with element stride x_row_stride (a strided view of the residual stream is fine); a bf16 [T][256]
 * or NULL (then x_new is not written and h = LayerNorm(x)); x_new f32 [T][256]; h bf16 [T][256]; mean, rstd f32 [T]
 * (saved for the backward).  seed, seed_state: as for g2048_attn_fwd; pass the same pair to the backward.
 * gamma NULL: no LayerNorm, h = bf16(x + dropout(a)) (the output of the LAST sub-layer, which the heads read in bf16);
 * beta, mean, rstd and x_new may then be NULL too. */
int g2048_add_ln_fwd(const float *x, int64_t x_row_stride, const void *a, const float *gamma, const float *beta,
                     float *x_new, void *h, float *mean, float *rstd, int64_t T, float eps, float p_drop,
                     uint64_t seed, const uint64_t *seed_state, void *stream);
/* x_norm = the tensor that was normalised (x_new, or x when a was NULL); g_x f32 or NULL = gradient arriving on x_new from
 * the residual stream: [T][256] with g_x_period 1, or only for every g_x_period-th token row ([T / g_x_period][256], e.g.
 * period 17 = the CLS rows of [B][17][256], all the last encoder layer hands back; T must then be a multiple of g_x_period, otherwise
 * G2048_EINVAL: the token row g_x_period * (T / g_x_period) would read behind g_x); g_h bf16 [T][256].  dx f32 [T][256] = g_x + dLayerNorm (gradient for x);
 * da bf16 [T][256] or NULL = dropout-masked dx (gradient for a); dparams f32 [3][256] = dgamma, dbeta and the column
 * sums of da (= the bias gradient of the Linear that produced a; zeros when da is NULL), summed in a fixed order;
 * workspace: g2048_add_ln_bwd_workspace_floats(T) floats of scratch.  dparams NULL: first stage only, the workspace then
 * holds f32 [workspace floats / 768][3 * 256] partial sums (dgamma | dbeta | bias gradient) for g2048_reduce_jobs.
 * gamma NULL (the forward ran without LayerNorm): dx = g_x + g_h, dgamma = dbeta = 0; x_norm, mean, rstd are not read. */
int64_t g2048_add_ln_bwd_workspace_floats(int64_t T);
int g2048_add_ln_bwd(const float *x_norm, int64_t x_row_stride, const float *g_x, const void *g_h, const float *mean,
                     const float *rstd, const float *gamma, float *dx, void *da, float *dparams, float *workspace,
                     int64_t T, float p_drop, uint64_t seed, const uint64_t *seed_state, int g_x_period, void *stream);

/* ---- policy network (update): Linear (256 outputs) fused with the add + LayerNorm kernel behind it -------------- */

/* x_new = x + dropout(u . W^T + bias);  h = bf16(LayerNorm(x_new) * gamma + beta) in ONE launch: g2048_linear_bf16 (N = 256)
 * followed by g2048_add_ln_fwd, without the bf16 [T][256] tensor between them (reference: `x = x + dropout1(self_attn(...))` /
 * `x = x + dropout2(linear2(...))` + the next sub-layer's norm, nn.TransformerEncoderLayer(norm_first=True) built at
 * src/ppo/transformer_encoder.py:138-148).  u bf16 [T][K], leading dimension ldu (elements, multiple of 8); w_packed: the Linear's
 * weight [256][K] as bf16 in the FRAGMENT-PACKED layout above (g2048_opt_step maintains such copies); K = 256, 512, 768 or 1024; bias f32 [256]
 * or NULL; the rest as g2048_add_ln_fwd (same dropout hash on the same element index: the two paths draw the same mask for the same
 * seed).  The Linear's output is rounded to bf16 before dropout and the add, as the unfused pair does. */
int g2048_linear_add_ln_fwd(const void *u, int64_t ldu, const void *w_packed, const float *bias, int K, const float *x,
                            int64_t x_row_stride, const float *gamma, const float *beta, float *x_new, void *h, float *mean,
                            float *rstd, int64_t T, float eps, float p_drop, uint64_t seed, const uint64_t *seed_state, void *stream);
/* g_h = bf16(dy . Wt^T);  then g2048_add_ln_bwd on it: the input-gradient GEMM of the Linear that CONSUMED h (linear1: K = 1024,
 * in_proj: K = 768) fused with the backward of the LayerNorm that produced h (reference: autograd of the same modules).
 * dy bf16 [T][K]; wt_packed: the TRANSPOSE of that Linear's weight, [256][K], fragment-packed - or K consecutive columns of a wider
 * packed matrix [256][K'] (point at the first k-step and pass wt_tile_stride = (K' / 16) * 512, the distance in elements between its
 * 32-row tiles; 0 = dense): the K/V rows of a packed in_proj^T.  g_h_extra (bf16 [T / extra_period][256] or NULL) is added to g_h on
 * the rows tok % extra_period == 0 (rounded to bf16 again, as an addmm into the bf16 gradient would): the CLS rows' share of the
 * last layer's query projection.  G2048_EINVAL when g_x is given and T is no multiple of g_x_period, or g_h_extra is given and T is no
 * multiple of extra_period (the last token row of that kind would read behind the buffer).  da may be NULL (the LayerNorm had no branch); partial: f32
 * [g2048_linear_add_ln_bwd_partial_rows(T)][3][256] first-stage sums (dgamma | dbeta | column sums of da) for g2048_reduce_jobs. */
int64_t g2048_linear_add_ln_bwd_partial_rows(int64_t T);
int g2048_linear_add_ln_bwd(const void *dy, int64_t lddy, const void *wt_packed, int64_t wt_tile_stride, int K, const float *x_norm,
                            int64_t x_row_stride, const float *g_x, int g_x_period, const void *g_h_extra, int extra_period,
                            const float *mean, const float *rstd, const float *gamma, float *dx, void *da, float *partial, int64_t T,
                            float p_drop, uint64_t seed, const uint64_t *seed_state, void *stream);

/* ---- MLP policy (BASELINE configs[1]): the update as a handful of launches ---------------------------------------------- */

/* trunk_in on packed boards: y[m] = relu(bias + sum over the 16 cells c of wt[31 c + min(boards[m][c], 30)]) (bf16 [M][512]; an
 * exponent above 30 counts as class 30, in y and in onehot) - a one-hot input times W^T is a sum of weight columns (reference: the MLP policy has no counterpart in the reference; its input convention is the
 * one-hot observation of src/runs/batch_runner.py:130-136).  wt: bf16 [496][512], the TRANSPOSE of the Linear's weight [512][496];
 * bias f32 [512]; onehot (bf16 [M][512], columns 496.. zero; may be NULL): the one-hot matrix itself, which the weight-gradient launch
 * multiplies with. */
int g2048_mlp_embed_fwd(const uint8_t *boards, const void *wt, const float *bias, void *y, void *onehot, int64_t M, void *stream);

/* A table of small GEMMs in ONE launch: for every job y[M][N] (bf16) = epi(sum over its K-segments s of x[s][M][k[s]] . w[s][N][k[s]]^T),
 * bf16 operands, f32 accumulation; epi: + bias (f32 [N], or NULL), ReLU when relu != 0, multiplied by (act > 0) when act (bf16 [M][N],
 * leading dimension ldact) is given - the ReLU backward on a saved activation.  Two K-segments: two Linears back-propagating into the
 * same input.  Replaces nn.Linear + ReLU and their autograd for 2048-row activations, where a hipGraph node costs more than its
 * arithmetic.  N, k[s] multiples of 64 (k[1] may be 0); leading dimensions multiples of 8 (ldact: 4); bases 16-byte aligned (act: 8).
 * jobs: host array, read during the call. */
#define G2048_GEMM_MAX_JOBS 8
typedef struct {
    const void *x[2]; int64_t ldx[2];
    const void *w[2]; int64_t ldw[2];
    int32_t k[2];
    const float *bias;
    const void *act; int64_t ldact;
    void *y; int64_t ldy;
    int32_t N, relu;
} g2048_gemm_job;
int g2048_gemm_jobs(const g2048_gemm_job *jobs, int n_jobs, int64_t M, void *stream);

/* Both heads' output layers: logits[m][0..3] = h2[m][:512] . w3[0..3]^T, values[m] = h2[m][512:] . w3[4]  (h2 bf16 [M][1024] = the
 * actor's | the critic's last hidden layer; w3 bf16 [5][512] = actor.4.weight, then critic.4.weight: src/ppo/ppo_agent.py:72-87). */
int g2048_mlp_out_fwd(const void *h2, const void *w3, float *logits, float *values, int64_t M, void *stream);
/* Their backward: dh2 (bf16 [M][1024]) = [w3[0..3]^T dlogits | w3[4] dvalues] where h2 > 0; partial: f32
 * [g2048_mlp_out_bwd_partial_rows(M)][5][512] first-stage sums of the output layers' weight gradients (for g2048_reduce_jobs). */
int64_t g2048_mlp_out_bwd_partial_rows(int64_t M);
int g2048_mlp_out_bwd(const float *dlogits, const float *dvalues, const void *h2, const void *w3, void *dh2, float *partial, int64_t M,
                      void *stream);

/* ---- policy network (update): bias gradients ------------------------------------------------------------ */

/* out[c] = sum_r x[r][c] for x bf16 (is_bf16 != 0) or f32 [T][N] with element stride row_stride between rows; f32
 * accumulation in a fixed order (bit-reproducible, safe to replay from a hipGraph).  N a multiple of 4 (matrices wider
 * than 1024 columns are summed in column tiles of 1024), row_stride >= N.
 * The bias gradient of every Linear in the update, and the CLS-token gradient (reference: nn.Linear inside
 * src/ppo/transformer_encoder.py:138-148 and src/ppo/ppo_agent.py:59-86; PyTorch computes it with at::sum).
 * workspace: g2048_colsum_workspace_floats(T, N) floats of scratch.  out NULL (N <= 1024 only): first stage only, the
 * workspace then holds f32 [g2048_colsum_partial_rows(T, N)][N] partial sums for g2048_reduce_jobs. */
#define G2048_COLSUM_MAX_GROUPS 512
int64_t g2048_colsum_workspace_floats(int64_t T, int N);
int64_t g2048_colsum_partial_rows(int64_t T, int N);
int g2048_colsum(const void *x, int is_bf16, int64_t row_stride, int64_t T, int N, float *workspace, float *out,
                 void *stream);

/* ---- PPO update: loss ------------------------------------------------------------------------------------- */

/* Clipped-surrogate PPO loss of one minibatch, forward + gradient in one launch (reference:
 * PPOTrainer._compute_ppo_loss src/ppo/ppo_trainer.py:251-314 over PPOAgent.evaluate_actions src/ppo/ppo_agent.py:159-191).
 * logits [M][4] and values [M]: f32, or bf16 when the *_bf16 flag is set; actions u8 [M] (0..3); mask_bits u8 [M]
 * (bit a = action a legal) or NULL for no masking; old_logp, adv, ret f32 [M].
 * Out: new_logp f32 [M]; sums f32 [5] = mean policy loss, mean value loss, mean entropy loss (-H), mean total loss,
 * mean(old_logp - new_logp); dlogits [M][4] and dvalues [M] = d(mean total loss)/d(input) in the input's dtype.
 * total = policy + c_value * value + c_entropy * entropy_loss.  One workgroup, fixed summation order.
 * grad_scale (optional device f32 scalar, e.g. GradScaler's scale): dlogits and dvalues come out multiplied by it, i.e. as
 * the gradients of grad_scale * total (scaler.scale(loss).backward() of the reference, src/ppo/ppo_trainer.py:411-413).
 * running (optional device f64 [5]): running[k] += (double)sums[k] - the per-update accumulation of the logged means
 * (src/ppo/ppo_trainer.py:424-437 of the reference sums Python floats) without a launch of its own per minibatch. */
#define G2048_PPO_LOSS_MAX_BATCH 1048576
int g2048_ppo_loss(const void *logits, int logits_bf16, const void *values, int values_bf16, const uint8_t *actions,
                   const uint8_t *mask_bits, const float *old_logp, const float *adv, const float *ret, int64_t M,
                   float clip_eps, float c_value, float c_entropy, float *new_logp, float *sums, void *dlogits,
                   void *dvalues, const float *grad_scale, double *running, void *stream);

/* ---- imitation update: loss ---------------------------------------------------------------------------------
 * Cross-entropy of the policy to a teacher's action scores (no reference counterpart: the reference only trains by PPO).  Per
 * sample, with z_j = logit_j, or logit_j - 1e8 where action j is illegal (g2048_ppo_loss's convention):
 *   pi = softmax(z), lp = log pi, ent = -sum_j lp_j pi_j
 *   a* = the first maximum over j of teacher_q_j - (legal ? 0 : 1e8), in f32 (the engine's masked argmax)
 *   p* = one-hot at a* for tau == 0; for tau > 0 p*_j = exp((q_j - q_a*) / tau) / sum over the legal j, 0 where illegal
 *   ce = -sum over the legal j of p*_j lp_j, vl = (V - value_target)^2, el = -ent, tot = ce + c_value vl + c_entropy el
 *   d tot / d z_j = (pi_j - p*_j) + c_entropy pi_j (lp_j + ent),  d tot / d V = 2 c_value (V - value_target)
 * A sample without a legal action (mask_bits == 0) is all zeros - losses, agreement, new_logp and gradients - but counts in M. */

/* The f32 elements of workspace that g2048_distill_loss needs, 5 per 256 samples; -1 for M < 1 or M > G2048_PPO_LOSS_MAX_BATCH. */
int64_t g2048_distill_loss_workspace_floats(int64_t M);

/* logits [M][4] and values [M]: f32, or bf16 when the *_bf16 flag is set; mask_bits u8 [M] (bit a = action a legal) or NULL for
 * no masking; teacher_q f32 [M][4]; value_target f32 [M].  values, value_target and dvalues are NULL together: no critic term,
 * sums[1] = 0 and dvalues is not touched.
 * Out: new_logp f32 [M] = lp[a*]; sums f32 [5] = mean ce, mean vl, mean el, mean tot, mean agreement (1 where the first maximum
 * of z is a*); dlogits [M][4] and dvalues [M] = d(mean tot)/d(input) in the input's dtype, multiplied by grad_scale (optional
 * device f32 scalar) as in g2048_ppo_loss; running (optional device f64 [5]): running[k] += (double)sums[k].
 * Two launches: one sample per lane in ceil(M / 256) workgroups whose five partial sums go to workspace, then one workgroup that
 * adds them in ascending workgroup order.  No floating-point atomics: the same inputs give the same bits on any device.
 * G2048_EINVAL, before any device work: a null logits, teacher_q, new_logp, sums, dlogits or workspace; values, value_target
 * and dvalues not all null or all given; M for which g2048_distill_loss_workspace_floats returns -1; tau negative or not finite;
 * teacher_q not 16-byte aligned, running not 8-byte aligned, a bf16 array not 2-byte or any other array not 4-byte aligned. */
int g2048_distill_loss(const void *logits, int logits_bf16, const void *values, int values_bf16, const uint8_t *mask_bits,
                       const float *teacher_q, const float *value_target, int64_t M, float tau, float c_value, float c_entropy,
                       float *new_logp, float *sums, void *dlogits, void *dvalues, const float *grad_scale, double *running,
                       float *workspace, void *stream);

/* Row i of the minibatch = row idx[i] (int64, clamped to [0, N)) of the imitation ring: boards u8 [N][16], masks u8 [N],
 * teacher_q f32 [N][4], value_target f32 [N] (NULL together with o_vt) -> the o_* arrays of M rows.  One launch; a board moves as
 * one 16-byte word and the four scores as another.
 * G2048_EINVAL: a null pointer other than that pair, value_target and o_vt not both null or both given, M < 1, N < 1, boards,
 * o_boards, teacher_q or o_q not 16-byte aligned, idx not 8-byte aligned, value_target or o_vt not 4-byte aligned. */
int g2048_distill_gather(const int64_t *idx, int64_t M, int64_t N, const uint8_t *boards, const uint8_t *masks, const float *teacher_q,
                         const float *value_target, uint8_t *o_boards, uint8_t *o_masks, float *o_q, float *o_vt, void *stream);

/* ---- policy network (update): feed-forward activation ---------------------------------------------------- */

/* y = dropout(relu(x)), x and y bf16 [T][F] (F a multiple of 8, F <= 2048): `dropout(activation(linear1(x)))` of the
 * encoder layer's feed-forward block (reference: nn.TransformerEncoderLayer, src/ppo/transformer_encoder.py:138-148).
 * seed, seed_state: as for g2048_attn_fwd. */
int g2048_relu_dropout_fwd(const void *x, void *y, int64_t T, int F, float p_drop, uint64_t seed,
                           const uint64_t *seed_state, void *stream);
/* dx = dy / (1 - p_drop) where y != 0, else 0 (y is non-zero exactly where the unit was active and kept: neither x nor
 * a mask is needed); dbias f32 [F] = column sums of dx in a fixed order = the bias gradient of the Linear in front.
 * dx may alias dy.  workspace: g2048_relu_dropout_bwd_workspace_floats(T, F) floats.  dbias NULL: first stage only, the
 * workspace then holds f32 [workspace floats / F][F] partial sums for g2048_reduce_jobs. */
int64_t g2048_relu_dropout_bwd_workspace_floats(int64_t T, int F);
int g2048_relu_dropout_bwd(const void *dy, const void *y, void *dx, float *dbias, float *workspace, int64_t T, int F,
                           float p_drop, void *stream);

/* ---- policy network (update): weight gradient of a Linear over the whole minibatch ------------------------------ */

/* parts[s][n][k] = sum over the tokens t of slice s (T / slices consecutive rows) of dy[t][n] * x[t][k]: the first stage of
 * dW = dY^T X for an nn.Linear applied to T token rows (reference: autograd of the Linears of nn.TransformerEncoderLayer,
 * src/ppo/transformer_encoder.py:138-148, inside PPOTrainer.update_policy, src/ppo/ppo_trainer.py:409-437); the sum over s is
 * left to g2048_reduce_jobs.  dy bf16 [T][N] and x bf16 [T][K] with leading dimensions lddy / ldx (elements, multiples of 8),
 * parts bf16 [slices][N][K] contiguous; N and K multiples of 128, T a multiple of 64 * slices, slices 1..7 or a multiple of
 * 8; base pointers 16-byte aligned.  f32 accumulation over a slice, one rounding to bf16 per partial.  block_rows: rows of the
 * gradient per workgroup (x 128 columns), 128 or 256 (N a multiple of 256), 0 = the kernel's choice; slices x blocks workgroups.
 * colsum (optional): f32 [slices][N], colsum[s][n] = sum over the slice's tokens of dy[t][n] (f32 sum of the bf16 values) - the
 * first stage of the Linear's bias gradient `dy.sum(0)`, read off the operand tiles the product stages anyway. */
int g2048_dweight_bf16(const void *dy, int64_t lddy, const void *x, int64_t ldx, void *parts, float *colsum, int64_t T, int N,
                       int K, int slices, int block_rows, void *stream);

/* The same for several Linears in ONE launch (the weight gradients of a whole backward pass, deferred to its end by the caller):
 * job j computes what g2048_dweight_bf16(dy, lddy, x, ldx, parts, colsum, T, N, K, slices, 128) does, bit for bit, with slices a multiple
 * of 8.  jobs: host array, read during the call.  parts_f32 != 0: the job's partials are stored as f32 [slices][N][K] instead of bf16
 * (twice the bytes into g2048_reduce_jobs; the switch behind profiles/round4_dweight_slices_seeds.txt).
 * Block shapes: a job whose N and K are multiples of 256 is cut into [256 x 256] cells, row-major; its first n_big cells are one
 * [256 x 256] block each (1.5 transposed LDS reads per MFMA instead of 3), every other cell four [128 x 128] blocks; all [256 x 256]
 * blocks of the launch come first in the grid.  g2048_dweight_jobs_plan writes n_big[j] for a launch on `cus` compute units (host
 * arithmetic only; the pointers of the jobs are not read): big_cells >= 0 deals that many cells to the jobs in order, big_cells < 0 is
 * the launch's own choice - whole rounds of the chip in [256 x 256] blocks, the remainder in [128 x 128] blocks where that is at most
 * two rounds of them.  g2048_dweight_jobs_tiled launches with that plan (big_cells < 0: for the current device's CU count);
 * g2048_dweight_jobs is g2048_dweight_jobs_tiled with big_cells = -1.  The partials do not depend on the plan. */
#define G2048_DWG_MAX_JOBS 16
typedef struct {
    const void *dy; const void *x; void *parts; float *colsum;
    int64_t lddy, ldx, T;
    int32_t N, K, slices, parts_f32;
} g2048_dwg_job;
int g2048_dweight_jobs(const g2048_dwg_job *jobs, int n_jobs, void *stream);
int g2048_dweight_jobs_tiled(const g2048_dwg_job *jobs, int n_jobs, int big_cells, void *stream);
int g2048_dweight_jobs_plan(const g2048_dwg_job *jobs, int n_jobs, int big_cells, int cus, int32_t *n_big);

/* ---- policy network (update): Linear for tall-skinny activations ------------------------------------------ */

/* y[T][N] = x[T][K] . weight[N][K]^T (+ bias[N]) - nn.Linear in bf16 with f32 accumulation (reference: every nn.Linear
 * of nn.TransformerEncoderLayer, src/ppo/transformer_encoder.py:138-148, and the same product with weight^T for the
 * input gradient).  x, weight, y bf16 with leading dimensions ldx, ldw, ldy (elements, multiples of 8); bias f32 or
 * NULL; K and N multiples of 128; all base pointers 16-byte aligned. */
int g2048_linear_bf16(const void *x, int64_t ldx, const void *weight, int64_t ldw, const float *bias, void *y, int64_t ldy,
                      int64_t T, int K, int N, void *stream);

/* y = dropout(relu(x . weight^T + bias)) in one launch: linear1 + activation + dropout of the encoder layer's feed-forward
 * block (reference: nn.TransformerEncoderLayer._ff_block, built at src/ppo/transformer_encoder.py:138-148).  Operands as
 * for g2048_linear_bf16 with K <= 256 and bias required; the pre-activation is never rounded to bf16.  seed / seed_state
 * as for g2048_attn_fwd.  The output is non-zero exactly where the unit was active and kept; mask_bits (optional,
 * g2048_ffn_mask_bytes(T, N) bytes, 8-byte aligned) receives one bit per output saying so, in an opaque layout that only
 * g2048_linear_mask_bwd_bf16 with the same T and N reads. */
int64_t g2048_ffn_mask_bytes(int64_t T, int N);
int g2048_linear_relu_dropout_bf16(const void *x, int64_t ldx, const void *weight, int64_t ldw, const float *bias, void *y,
                                   int64_t ldy, int64_t T, int K, int N, float p_drop, uint64_t seed,
                                   const uint64_t *seed_state, void *mask_bits, void *stream);
/* The backward of `y = dropout(relu(.)); out = y . W2^T` with respect to the pre-activation, in one GEMM:
 * dz[T][N] = (dy[T][K] . weight_t[N][K]^T) / (1 - p_drop) where y != 0 (mask_bits of the forward call), else 0
 * (weight_t = W2^T, i.e. linear2's weight [K][N] transposed to [N][K]; dy = the gradient of linear2's output), and
 * dbias f32 [N] = column sums of the bf16 dz in a fixed order = linear1's bias gradient.  Replaces g2048_linear_bf16 +
 * g2048_relu_dropout_bwd (which re-reads the [T][N] activation; the bit mask is 1/16 of it).  K <= 256;
 * workspace: g2048_linear_mask_bwd_workspace_floats(T, N) floats; dbias NULL: first stage only, the workspace then holds
 * f32 [g2048_linear_mask_bwd_partial_rows(T, N)][N] partial sums for g2048_reduce_jobs. */
int64_t g2048_linear_mask_bwd_workspace_floats(int64_t T, int N);
int64_t g2048_linear_mask_bwd_partial_rows(int64_t T, int N);
int g2048_linear_mask_bwd_bf16(const void *dy, int64_t lddy, const void *weight_t, int64_t ldw, const void *mask_bits, void *dz,
                               int64_t lddz, float *dbias, float *workspace, int64_t T, int K, int N, float p_drop,
                               void *stream);

/* ---- policy network (update): token embedding of packed boards ---------------------------------------------- */

/* x0[m][0] = cls, x0[m][1 + c] = dropout(wt[boards[m][c]] + pe[c]): the bias-free input Linear over the one-hot cell (w_ld
 * = 0: wt = input_embedding.weight^T, f32 [31][256], 16-byte aligned; w_ld >= 31: wt = the nn.Linear weight itself, f32
 * [256][w_ld], read in place), the 2-D positional code (pe f32 [16][256]) and the CLS concat
 * (reference: src/ppo/ppo_agent.py:59-66,103-106; src/ppo/transformer_encoder.py:150-190).  boards u8 [M][16] with
 * cells <= 30, x0 f32 [M][17][256].  The positional encoding's dropout (p_drop; seed, seed_state as for g2048_attn_fwd)
 * applies to the 16 board tokens, not to the CLS row. */
int g2048_embed_fwd(const uint8_t *boards, const float *wt, int w_ld, const float *pe, const float *cls, float *x0, int64_t M,
                    float p_drop, uint64_t seed, const uint64_t *seed_state, void *stream);
/* dwt_dcls f32 [32][256]: rows 0..30 = gradient of wt (sum of dx0 rows by cell value), row 31 = gradient of cls; fixed
 * summation order.  dx0 f32 [M][17][256]; workspace: g2048_embed_bwd_workspace_floats(M) floats.  dwt_dcls NULL: first
 * stage only, the workspace then holds f32 [workspace floats / 8192][32 * 256] partial sums for g2048_reduce_jobs (whose
 * transpose_rows = 31 stores the first 31 * 256 columns as the [256][31] gradient of the nn.Linear weight). */
/* The same, and on the row it still holds h[m][t] = bf16(LayerNorm(x0[m][t]) * gamma + beta) with mean / rstd f32 [M * 17]: the first
 * LayerNorm of the encoder (layers[0].norm1, src/ppo/transformer_encoder.py:138-148 norm_first) in g2048_add_ln_fwd's arithmetic, without
 * reading x0 back.  gamma, beta f32 [256]; h bf16 [M][17][256]. */
int g2048_embed_ln_fwd(const uint8_t *boards, const float *wt, int w_ld, const float *pe, const float *cls, float *x0, int64_t M,
                       float p_drop, uint64_t seed, const uint64_t *seed_state, const float *gamma, const float *beta, float eps,
                       void *h, float *mean, float *rstd, void *stream);
int64_t g2048_embed_bwd_workspace_floats(int64_t M);
int g2048_embed_bwd(const uint8_t *boards, const float *dx0, float *dwt_dcls, float *workspace, int64_t M, float p_drop,
                    uint64_t seed, const uint64_t *seed_state, void *stream);

/* ---- PPO update: minibatch assembly ------------------------------------------------------------------------ */

/* ---- gradient reductions of the update, second stage ----------------------------------------------------------- */

/* All second-stage reductions of one backward pass in one launch (per 64 jobs): for every job,
 * dst[c] = sum over p < parts of src[p * part_stride + c], c < n, in f32 and in a fixed order.  Jobs: the 16 split-K
 * slices of a weight gradient (bf16 [16][out * in]), the per-workgroup partial column sums the backward kernels leave in
 * their workspace when called with a NULL result pointer (g2048_add_ln_bwd, g2048_relu_dropout_bwd,
 * g2048_linear_mask_bwd_bf16, g2048_embed_bwd, g2048_colsum: f32 [rows][N], rows = workspace floats / N), a bf16 -> f32
 * conversion (parts 1).  Replaces what PyTorch runs as one at::sum / copy kernel per parameter
 * (reference: loss.backward() at src/ppo/ppo_trainer.py:410-414).  jobs: host array, read during the call; src 2- (bf16) or
 * 4-byte aligned device memory, vector loads when 8-/16-byte aligned with part_stride % 4 == 0.
 * transpose_rows = R > 0 (n a multiple of R): the n columns are a row-major [R][n / R] matrix and the sum is stored
 * transposed, dst[(c % (n / R)) * R + c / (n / R)] - the embedding gradient is accumulated per class ([31][256]) and belongs
 * to an nn.Linear weight ([256][31]); 0: dst[c]. */
#define G2048_REDUCE_MAX_JOBS 64
typedef struct {
    const void *src; float *dst; int64_t part_stride; int32_t n, parts, src_bf16, transpose_rows;
} g2048_reduce_job;
int g2048_reduce_jobs(const g2048_reduce_job *jobs, int n_jobs, void *stream);

/* ---- optimiser step (update) ---------------------------------------------------------------------------- */

/* One optimiser step for every parameter of the agent in two launches: GradScaler unscale + inf check, gradient-norm
 * clipping, AdamW, GradScaler update (reference: src/ppo/ppo_trainer.py:413-434 = scaler.unscale_(opt);
 * clip_grad_norm_(params, max_grad_norm); scaler.step(opt); scaler.update(), with opt = torch.optim.AdamW built by
 * src/optim/configure_optimizers.py:16-127).
 * grads / exp_avg / exp_avg_sq: flat f32 device buffers (16-byte aligned) sharing one element layout; chunks[n_chunks]
 * (device memory): piece `n` <= G2048_OPT_CHUNK elements of one parameter tensor starting at `param` (16-byte aligned),
 * whose gradient and moments start at element `offset` (a multiple of 4) of the flat buffers, hyper-parameters
 * groups[group].  groups: host array, read during the call (the LR schedule changes lr every step).
 * A chunk may name bf16 shadows of its tensor (what the bf16 update path multiplies with): they are rewritten together with
 * the parameter, so that no cast kernels run per step.
 * max_grad_norm <= 0: no clipping.  steps: device f32 [n_steps], the number of steps taken so far, one copy per parameter
 * tensor as torch.optim keeps them (all equal; every entry +1 per non-skipped call).
 * scale / growth_tracker: the GradScaler's device scalars, or NULL/NULL when no scaler is used (then gradients are taken
 * as they are and nothing is skipped); with a scaler, a step whose gradients hold an inf/nan changes neither parameters
 * nor moments nor steps, and the scale is multiplied by backoff; after growth_interval consecutive clean steps by growth.
 * workspace: g2048_opt_workspace_floats(n_chunks) floats.  info (optional, device f32[2]): total gradient norm before clipping, found_inf.
 * Arithmetic is torch's fused AdamW (bias corrections in f64 from the step count); the summation order of the norm is
 * fixed by the chunk table. */
#define G2048_OPT_CHUNK 2048
#define G2048_OPT_MAX_GROUPS 4
typedef struct {
    float *param; int64_t offset; int32_t n; int32_t group;
    void *shadow;      /* optional bf16 copy of the tensor (dense, same element order): the chunk's piece is refreshed in place */
    void *shadow_t;    /* optional bf16 copy of the TRANSPOSED 2-D tensor [cols][rows] */
    void *shadow_p;    /* optional bf16 copy of the 2-D tensor in the fragment-packed layout (see g2048_tail_saved); rows % 32 == 0, cols % 16 == 0 */
    void *shadow_tp;   /* optional fragment-packed bf16 copy of the TRANSPOSED tensor; cols % 32 == 0, rows % 16 == 0 */
    int32_t e0;        /* element index of the chunk's first element inside its tensor */
    int32_t rows, cols; /* shape of the 2-D tensor (only read when shadow_t is set) */
    int32_t reserved;
} g2048_opt_chunk;
typedef struct { double lr, beta1, beta2, eps, weight_decay; } g2048_opt_group; /* f64, as torch.optim holds them */
int64_t g2048_opt_workspace_floats(int n_chunks);
int g2048_opt_step(const g2048_opt_chunk *chunks, int n_chunks, const float *grads, float *exp_avg, float *exp_avg_sq,
                   const g2048_opt_group *groups, int n_groups, float max_grad_norm, float *steps, int n_steps, float *scale,
                   int32_t *growth_tracker, float growth, float backoff, int growth_interval, float *workspace,
                   float *info, void *stream);

/* The same step with the reference's LAMB optimiser (src/optim/lamb.py:106-209 inside the update loop of
 * src/ppo/ppo_trainer.py:413-434: scaler.unscale_(opt); clip_grad_norm_(params, max_grad_norm); scaler.step(Lamb);
 * scaler.update()), in three launches over the same chunk table, flat buffers, scaler scalars and info as g2048_opt_step:
 *   g = grad * inv_scale;  norm = ||g|| over all chunks;  c1 = min(1, max_grad_norm / (norm + 1e-6)) (max_grad_norm <= 0: 1);
 *   c2 = max(1, norm * c1 / lamb_max_grad_norm) (Lamb's own global clip, optimizer.defaults["max_grad_norm"]; <= 0: none.  The
 *   reference takes that norm again from the clipped elements; norm * c1 differs from it by rounding only and saves a pass);
 *   g' = g * c1 / c2, applied as grad * (float)(inv_scale * c1 / c2) with the factor formed in f64 from the f32 sum of squares and
 *   rounded once (two roundings per element where the reference's three passes have five);  m = beta1 * m + beta3 * g';  v = beta2 * v + (1 - beta2) * g'^2;
 *   u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + weight_decay * p   (bc1, bc2 in f64 from the step count; 1 without bias_correction);
 *   per TENSOR, when weight_decay != 0 or adapt: r = ||p|| / ||u|| if both are > 0, else 1; min(r, 1) with trust_clip; else r = 1;
 *   p -= lr * r * u, the chunk's bf16 shadows rewritten.
 * The chunks of one tensor must be adjacent and in ascending e0 order, with rows * cols = the tensor's element count (what
 * opt_chunk_table writes): the per-tensor norms are summed over them in that order.  beta3 = 1 - beta1 (grad_averaging) or 1.
 * steps: device f32 [n_steps], every entry +1 per non-skipped call; the bias corrections use steps[0] (Lamb keeps one count per
 * group, FlatLambStep one for all).  Skipping, scale / growth_tracker, info, argument checks and error codes: as g2048_opt_step.
 * workspace: g2048_lamb_workspace_floats(n_chunks) floats. */
typedef struct { double lr, beta1, beta2, beta3, eps, weight_decay;
                 int32_t bias_correction, adapt, trust_clip, reserved; } g2048_lamb_group;
int64_t g2048_lamb_workspace_floats(int n_chunks);
int g2048_lamb_step(const g2048_opt_chunk *chunks, int n_chunks, const float *grads, float *exp_avg, float *exp_avg_sq,
                    const g2048_lamb_group *groups, int n_groups, float max_grad_norm, float lamb_max_grad_norm,
                    float *steps, int n_steps, float *scale, int32_t *growth_tracker, float growth, float backoff,
                    int growth_interval, float *workspace, float *info, void *stream);

/* ---- policy network (update): the 2048-row tail as two kernels -------------------------------------------------- */

/* Everything after the last encoder layer's attention works on ONE row per board (the "cls" reduction reads only the CLS row
 * of the last layer): out_proj + dropout + residual + LayerNorm(norm2), linear1 + ReLU + dropout, linear2 + dropout +
 * residual, then the actor head (256 -> 512 -> 512 -> 4) and the critic head (256 -> 512 -> 512 -> 1)
 * (reference: nn.TransformerEncoderLayer(norm_first=True), src/ppo/transformer_encoder.py:138-148 and :150-190 for the CLS
 * read-out; the heads of src/ppo/ppo_agent.py:62-92, evaluated by evaluate_actions :159-191).  d_model 256, feed-forward
 * 1024, head width 512.  g2048_cls_tail_fwd runs that chain for M rows in one launch, g2048_cls_tail_bwd its backward, and
 * g2048_dweight_t all weight / bias gradients from the transposed operands the two leave behind.
 * Weights: bf16 copies in nn.Linear's [out][in] layout (16-byte aligned), biases and LayerNorm parameters f32. */
typedef struct {
    const void *wo, *w1, *w2;           /* out_proj [256][256], linear1 [1024][256], linear2 [256][1024]: packed */
    const void *a1, *a2, *a3;           /* actor  [512][256], [512][512] packed; [4][512] row-major (no bias) */
    const void *c1, *c2, *c3;           /* critic [512][256], [512][512] packed; [1][512] row-major (no bias) */
    const float *bo, *b1, *b2, *ab1, *ab2, *cb1, *cb2;
    const float *ln_g, *ln_b;           /* norm2 */
} g2048_tail_weights;
/* the backward multiplies with the TRANSPOSED weights ([in][out], bf16, packed; g2048_opt_step keeps such shadows current) */
typedef struct {
    const void *woT, *w1T, *w2T;        /* [256][256], [256][1024], [1024][256] */
    const void *a1T, *a2T, *a3;         /* [256][512], [512][512]; a3 as it is, [4][512] */
    const void *c1T, *c2T, *c3;         /* [256][512], [512][512]; c3 as it is, [1][512] */
    const float *ln_g;
} g2048_tail_weights_t;
/* Fragment-packed layout ("packed" below) of a bf16 matrix X[rows][cols], rows % 32 == 0, cols % 16 == 0 -- the order in
 * which a wavefront consumes X as an MFMA operand, one contiguous KB per wave-instruction:
 *   offset(row, col) = ((((row / 32) * (cols / 16) + col / 16) * 2 + (col / 8) % 2) * 32 + row % 32) * 8 + col % 8.
 * The weights of g2048_tail_weights / g2048_tail_weights_t (except a3, c3: row-major) and every transposed activation buffer
 * below are stored that way; g2048_opt_step maintains packed shadows of parameters (g2048_opt_chunk.shadow_p / shadow_tp). */
/* What the forward leaves for the backward and for the weight gradients.  ld = number of columns of every transposed
 * buffer, >= 32 * ceil(M / 32) and a multiple of 16 (the packed layout has ld / 16 k-steps per row tile; both entry points return
 * G2048_EINVAL otherwise, as g2048_dweight_t does; the product passes multiples of 32); columns M..32 * ceil(M / 32) - 1 are written
 * as zero, columns beyond that are not written: allocate the buffers zero-filled.
 * masks: u16 [ceil(M/32)][G2048_TAIL_MASK_TILES][64], one bit per element of an MFMA accumulator tile (private layout). */
#define G2048_TAIL_MASK_TILES 96
typedef struct {
    float *x_mid, *mean, *rstd;         /* f32 [M][256] residual after the attention block; LayerNorm statistics [M] */
    void *masks;
    void *oT, *h2T, *uT, *featsT;       /* bf16 [256][ld], [256][ld], [1024][ld], [256][ld]: inputs of out_proj, linear1, linear2, heads */
    void *a1T, *a2T, *c1T, *c2T;        /* bf16 [512][ld] each: hidden activations of the heads */
    int64_t ld;                         /* columns of every transposed buffer: a multiple of 16, >= 32 * ceil(M / 32) */
} g2048_tail_saved;
/* dY^T of every Linear (bf16, [out][ld]; dlT / dvT have 32 rows of which 4 / 1 are written: allocate them zero-filled) and
 * the LayerNorm gradient partials f32 [ceil(M/32)][2][256] (dgamma | dbeta per workgroup, for g2048_reduce_jobs). */
typedef struct {
    void *daoT, *dzT, *df2T;            /* out_proj [256][ld], linear1 [1024][ld], linear2 [256][ld] */
    void *da1T, *da2T, *dlT;            /* actor [512][ld], [512][ld], [32][ld] */
    void *dc1T, *dc2T, *dvT;            /* critic [512][ld], [512][ld], [32][ld] */
    float *ln_partial;
} g2048_tail_grads;
/* o: bf16 [M][256] attention output of the CLS rows; x_cls: f32 rows of 256 with element stride x_row_stride (the CLS rows
 * of the residual stream, read in place); logits f32 [M][4], values f32 [M].  Dropout as everywhere in the update: the mask
 * is a function of (seed, *seed_state, site, element); pass the same triple to the backward. */
int g2048_cls_tail_fwd(const void *o, const float *x_cls, int64_t x_row_stride, const g2048_tail_weights *W,
                       const g2048_tail_saved *S, float *logits, float *values, int64_t M, float eps, float p_drop, uint64_t seed,
                       const uint64_t *seed_state, void *stream);
/* dlogits f32 [M][4], dvalues f32 [M] -> d_o bf16 [M][256] (gradient of the attention output), dx_cls f32 [M][256]
 * (gradient of the residual CLS rows), G (see above). */
int g2048_cls_tail_bwd(const float *dlogits, const float *dvalues, const g2048_tail_weights_t *WT, const g2048_tail_saved *S,
                       const g2048_tail_grads *G, void *d_o, float *dx_cls, int64_t M, float p_drop, uint64_t seed,
                       const uint64_t *seed_state, void *stream);

/* Weight gradients from transposed operands, all jobs in one launch: for job j,
 * dw[s][n][k] = sum over the s-th of `slices` equal pieces of the row axis of dyT[n][m] * xT[k][m]   (f32 [slices][N][K]),
 * db[s][n]    = the same sum of dyT[n][m]                                                        (f32 [slices][N], or NULL);
 * dyT bf16 [N][ld], xT bf16 [K][ld], both packed; N a multiple of 32, K of 64, m (rows used, <= ld) a multiple of 16 * slices
 * (8 slices put each slice on one XCD).  The slices are
 * summed by g2048_reduce_jobs.  Replaces dY^T X (torch: `dy.t() @ x`) and the bias column sums in the backward of every
 * nn.Linear of the tail (reference: loss.backward() at src/ppo/ppo_trainer.py:410-414).  jobs: host array, read during the call. */
#define G2048_DW_MAX_JOBS 16
typedef struct { const void *dyT; const void *xT; float *dw; float *db; int32_t N, K; } g2048_dw_job;
int g2048_dweight_t(const g2048_dw_job *jobs, int n_jobs, int64_t ld, int64_t m, int slices, void *stream);

/* Row i of the minibatch = sample idx[i] (int64, clamped to [0, N)) of the device-resident rollout buffer: boards
 * u8 [N][16], actions u8 [N], masks u8 [N], logp / adv / ret f32 [N] -> the o_* arrays of M rows.  One launch for what
 * the reference's DataLoader collation does per field (PPODataset.__getitem__, src/ppo/data_loader.py). */
int g2048_gather_minibatch(const int64_t *idx, int64_t M, int64_t N, const uint8_t *boards, const uint8_t *actions,
                           const uint8_t *masks, const float *logp, const float *adv, const float *ret, uint8_t *o_boards,
                           uint8_t *o_actions, uint8_t *o_masks, float *o_logp, float *o_adv, float *o_ret, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* G2048_H */
