"""ctypes binding of libg2048.so (C ABI: include/g2048.h).

This is the only place the Python host side touches native code.  There is no CPU fallback: if the
library is missing, or a tensor is not on a HIP device, the call raises.  Argument types, structs and
constants are read from the header itself (``_abi.py``); this module holds the wrappers only.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from ._abi import NativeError, read as _read_header

_PKG_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
LIB_PATH = os.environ.get("G2048_LIB", os.path.join(_PKG_ROOT, "lib", "libg2048.so"))
HEADER_PATH = os.path.join(os.path.dirname(_PKG_ROOT), "include", "g2048.h")

# include/g2048.h, read once per process: name -> (restype, argtypes), C struct name -> ctypes.Structure, G2048_NAME -> int
PROTOTYPES, STRUCTS, CONSTANTS = _read_header(HEADER_PATH)
SIGNATURES = {name: argtypes for name, (_, argtypes) in PROTOTYPES.items()}

RNG_LEGACY, RNG_PARTITIONABLE = CONSTANTS["G2048_RNG_LEGACY"], CONSTANTS["G2048_RNG_PARTITIONABLE"]
POLICY_DRUL, POLICY_RANDOM = CONSTANTS["G2048_POLICY_DRUL"], CONSTANTS["G2048_POLICY_RANDOM"]
MAX_FUSED_STEPS = CONSTANTS["G2048_MAX_FUSED_STEPS"]

_i32, _i64, _vp = C.c_int, C.c_int64, C.c_void_p

_lib = None


def load() -> C.CDLL:
    """Load libg2048.so or raise; never falls back to anything else."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"libg2048.so not found at {LIB_PATH}: build it with "
                f"`python 2048-ppo-agent_amd/build.py` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the 2048 rollout engine."
            )
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = restype, argtypes
        if lib.g2048_abi_version() != CONSTANTS["G2048_ABI_VERSION"]:
            raise NativeError("libg2048.so ABI version mismatch")
        _lib = lib
    return _lib


def _check(rc: int, name: str):
    if rc != 0:
        raise NativeError(f"{name} failed with code {rc}"
                          + (" (invalid argument)" if rc == -1 else f" (hipError {-rc - 1000})"))


def _dev(t: torch.Tensor | None, dtype, numel: int | None, name: str, optional=False):
    if t is None:
        if optional:
            return None
        raise NativeError(f"{name}: tensor required")
    if not t.is_cuda:
        raise NativeError(f"{name}: expected a HIP device tensor, got {t.device} (no CPU path exists)")
    if t.dtype != dtype or not t.is_contiguous():
        raise NativeError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
    if numel is not None and t.numel() < numel:
        raise NativeError(f"{name}: needs {numel} elements, has {t.numel()}")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


u8, i32, i64, f32 = torch.uint8, torch.int32, torch.int64, torch.float32
# uint32 keys travel as int32 tensors (same bits); helpers below convert
KEY_DTYPE = torch.int32


def keys_from_numpy(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(device)


def keys_to_numpy(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------ host-only
def chain_keys(key: np.ndarray, n: int, rng_mode: int):
    """n x (key, sub = split(key)) on the host. Returns (new_key u32[2], subs u32[n,2])."""
    k = np.array(key, dtype=np.uint32).reshape(2).copy()
    subs = np.empty((n, 2), np.uint32)
    _check(load().g2048_chain_keys(k.ctypes.data, subs.ctypes.data, n, rng_mode), "g2048_chain_keys")
    return k, subs


# ------------------------------------------------------------------------------------------ device calls
def split(key, n: int, rng_mode: int, device) -> torch.Tensor:
    out = torch.empty((n, 2), dtype=KEY_DTYPE, device=device)
    _check(load().g2048_split(int(key[0]), int(key[1]), _dev(out, KEY_DTYPE, 2 * n, "out"), n, rng_mode,
                              _stream()), "g2048_split")
    return out


def init(keys, boards, masks, done, rng_mode: int):
    B = masks.numel()
    _check(load().g2048_init(_dev(keys, KEY_DTYPE, 2 * B, "keys"), _dev(boards, u8, 16 * B, "boards"),
                             _dev(masks, u8, B, "masks"), _dev(done, u8, B, "done"), B, rng_mode, _stream()),
           "g2048_init")


def step(boards, masks, done, actions, keys, rewards, rng_mode: int):
    B = masks.numel()
    _check(load().g2048_step(_dev(boards, u8, 16 * B, "boards"), _dev(masks, u8, B, "masks"),
                             _dev(done, u8, B, "done"), _dev(actions, i32, B, "actions"),
                             _dev(keys, KEY_DTYPE, 2 * B, "keys"), _dev(rewards, f32, B, "rewards"), B, rng_mode,
                             _stream()), "g2048_step")


def observe(boards, obs):
    B = boards.numel() // 16
    _check(load().g2048_observe(_dev(boards, u8, 16 * B, "boards"), _dev(obs, u8, 496 * B, "obs"), B, _stream()),
           "g2048_observe")


def act_drul(masks, actions):
    B = masks.numel()
    _check(load().g2048_act_drul(_dev(masks, u8, B, "masks"), _dev(actions, i32, B, "actions"), B, _stream()),
           "g2048_act_drul")


def act_random(keys, masks, actions, log_probs, rng_mode: int):
    B = masks.numel()
    _check(load().g2048_act_random(_dev(keys, KEY_DTYPE, 2 * B, "keys"), _dev(masks, u8, B, "masks"),
                                   _dev(actions, i32, B, "actions"), _dev(log_probs, f32, B, "log_probs"), B,
                                   rng_mode, _stream()), "g2048_act_random")


def act_logits(keys, logits, masks, use_mask, sample, actions, log_probs, rng_mode: int):
    B = masks.numel()
    _check(load().g2048_act_logits(_dev(keys, KEY_DTYPE, 2 * B, "keys"), _dev(logits, f32, 4 * B, "logits"),
                                   _dev(masks, u8, B, "masks"), int(bool(use_mask)), int(bool(sample)),
                                   _dev(actions, i32, B, "actions"), _dev(log_probs, f32, B, "log_probs"), B,
                                   rng_mode, _stream()), "g2048_act_logits")


def reset_fused(sub, boards, masks, done, ep_len, B_total: int, env0: int, rng_mode: int):
    B = masks.numel()
    _check(load().g2048_reset_fused(int(sub[0]), int(sub[1]), _dev(boards, u8, 16 * B, "boards"),
                                    _dev(masks, u8, B, "masks"), _dev(done, u8, B, "done"),
                                    _dev(ep_len, i32, B, "ep_len"), B, B_total, env0, rng_mode, _stream()),
           "g2048_reset_fused")


def rollout_fused(step_subs: np.ndarray, t0: int, boards, masks, done, ep_len, tr_boards, tr_meta, tr_rewards,
                  tr_logp, B_total: int, env0: int, policy: int, fill_frozen: bool, rng_mode: int, live_count):
    B = masks.numel()
    subs = np.ascontiguousarray(step_subs, np.uint32).reshape(-1, 4)
    n = subs.shape[0]
    need = (t0 + n) * B
    _check(load().g2048_rollout_fused(subs.ctypes.data, n, t0, _dev(boards, u8, 16 * B, "boards"),
                                      _dev(masks, u8, B, "masks"), _dev(done, u8, B, "done"),
                                      _dev(ep_len, i32, B, "ep_len"), _dev(tr_boards, u8, 16 * need, "tr_boards"),
                                      _dev(tr_meta, u8, need, "tr_meta"), _dev(tr_rewards, f32, need, "tr_rewards"),
                                      _dev(tr_logp, f32, need, "tr_logp", optional=True), B, B_total, env0, policy,
                                      int(bool(fill_frozen)), rng_mode, _dev(live_count, i32, 1, "live_count"),
                                      _stream()), "g2048_rollout_fused")


def policy_step(act_sub, step_sub, logits, values, use_mask, sample, t: int, boards, masks, done, ep_len, tr_boards,
                tr_meta, tr_rewards, tr_logp, tr_values, B_total: int, env0: int, fill_frozen: bool, rng_mode: int,
                live_count):
    B = masks.numel()
    need = (t + 1) * B
    _check(load().g2048_policy_step(int(act_sub[0]), int(act_sub[1]), int(step_sub[0]), int(step_sub[1]),
                                    _dev(logits, f32, 4 * B, "logits"), _dev(values, f32, B, "values"),
                                    int(bool(use_mask)), int(bool(sample)), t, _dev(boards, u8, 16 * B, "boards"),
                                    _dev(masks, u8, B, "masks"), _dev(done, u8, B, "done"),
                                    _dev(ep_len, i32, B, "ep_len"), _dev(tr_boards, u8, 16 * need, "tr_boards"),
                                    _dev(tr_meta, u8, need, "tr_meta"), _dev(tr_rewards, f32, need, "tr_rewards"),
                                    _dev(tr_logp, f32, need, "tr_logp"), _dev(tr_values, f32, need, "tr_values"),
                                    B, B_total, env0, int(bool(fill_frozen)), rng_mode,
                                    _dev(live_count, i32, 1, "live_count", optional=True), _stream()), "g2048_policy_step")


def policy_step_autoreset(act_sub, step_sub, logits, values, use_mask, sample, t: int, boards, masks, ep_len, tr_boards,
                          tr_meta, tr_rewards, tr_logp, tr_values, B_total: int, env0: int, rng_mode: int):
    """One lock-step of the fixed-horizon mode: every lane steps, a terminated lane starts its next episode at once."""
    B = masks.numel()
    need = (t + 1) * B
    _check(load().g2048_policy_step_autoreset(
        int(act_sub[0]), int(act_sub[1]), int(step_sub[0]), int(step_sub[1]), _dev(logits, f32, 4 * B, "logits"),
        _dev(values, f32, B, "values"), int(bool(use_mask)), int(bool(sample)), t, _dev(boards, u8, 16 * B, "boards"),
        _dev(masks, u8, B, "masks"), _dev(ep_len, i32, B, "ep_len"), _dev(tr_boards, u8, 16 * need, "tr_boards"),
        _dev(tr_meta, u8, need, "tr_meta"), _dev(tr_rewards, f32, need, "tr_rewards"), _dev(tr_logp, f32, need, "tr_logp"),
        _dev(tr_values, f32, need, "tr_values"), B, B_total, env0, rng_mode, _stream()), "g2048_policy_step_autoreset")


def reset_key(step_sub) -> np.ndarray:
    """jax.random.fold_in(step_sub, 0xFFFFFFFF): the reset sub-key of one lock-step of the fixed-horizon mode."""
    out = np.empty(2, np.uint32)
    _check(load().g2048_reset_key(int(step_sub[0]), int(step_sub[1]), out.ctypes.data), "g2048_reset_key")
    return out


def gae_tb_boot(tr_rewards, tr_values, tr_meta, last_values, tr_adv, tr_ret, T: int, B: int, gamma: float, lam: float):
    n = T * B
    _check(load().g2048_gae_tb_boot(_dev(tr_rewards, f32, n, "tr_rewards"), _dev(tr_values, f32, n, "tr_values"),
                                    _dev(tr_meta, u8, n, "tr_meta"), _dev(last_values, f32, B, "last_values"),
                                    _dev(tr_adv, f32, n, "tr_adv"), _dev(tr_ret, f32, n, "tr_ret"), T, B, float(gamma),
                                    float(lam), _stream()), "g2048_gae_tb_boot")


def gae_tb(tr_rewards, tr_values, ep_len, tr_adv, tr_ret, T: int, B: int, gamma: float, lam: float):
    n = T * B
    _check(load().g2048_gae_tb(_dev(tr_rewards, f32, n, "tr_rewards"), _dev(tr_values, f32, n, "tr_values"),
                               _dev(ep_len, i32, B, "ep_len"), _dev(tr_adv, f32, n, "tr_adv"),
                               _dev(tr_ret, f32, n, "tr_ret"), T, B, float(gamma), float(lam), _stream()),
           "g2048_gae_tb")


def gae_flat(rewards, values, terms, adv, ret, gamma: float, lam: float):
    N = rewards.numel()
    _check(load().g2048_gae_flat(_dev(rewards, f32, N, "rewards"), _dev(values, f32, N, "values"),
                                 _dev(terms, u8, N, "terms"), _dev(adv, f32, N, "adv"), _dev(ret, f32, N, "ret"), N,
                                 float(gamma), float(lam), _stream()), "g2048_gae_flat")


def compact(tr_boards, tr_meta, tr_rewards, tr_logp, tr_values, ep_len, offsets, out_boards, out_actions, out_masks,
            out_rewards, out_logp, out_values, out_terms, T: int, B: int, N: int, tr_adv=None, tr_ret=None, out_adv=None,
            out_ret=None):
    n = T * B
    _check(load().g2048_compact(
        _dev(tr_boards, u8, 16 * n, "tr_boards"), _dev(tr_meta, u8, n, "tr_meta"),
        _dev(tr_rewards, f32, n, "tr_rewards"), _dev(tr_logp, f32, n, "tr_logp", optional=True),
        _dev(tr_values, f32, n, "tr_values", optional=True), _dev(tr_adv, f32, n, "tr_adv", optional=True),
        _dev(tr_ret, f32, n, "tr_ret", optional=True), _dev(ep_len, i32, B, "ep_len"),
        _dev(offsets, i64, B, "offsets"), _dev(out_boards, u8, 16 * N, "out_boards"),
        _dev(out_actions, u8, N, "out_actions"), _dev(out_masks, u8, N, "out_masks"),
        _dev(out_rewards, f32, N, "out_rewards"), _dev(out_logp, f32, N, "out_logp", optional=True),
        _dev(out_values, f32, N, "out_values", optional=True), _dev(out_adv, f32, N, "out_adv", optional=True),
        _dev(out_ret, f32, N, "out_ret", optional=True), _dev(out_terms, u8, N, "out_terms"), T, B,
        _stream()), "g2048_compact")


def policy_encoder_workspace_bytes(B: int) -> int:
    return int(load().g2048_policy_encoder_workspace_bytes(B))


def policy_encoder(boards, embed_table, cls_token, weights_bf16, params_f32, n_layers: int, features, workspace=None):
    """workspace: None (single kernel) or a uint8 device tensor of policy_encoder_workspace_bytes(B) bytes (the last
    layer then runs CLS-only in a second kernel)."""
    B = boards.numel() // 16
    if workspace is not None:
        need = policy_encoder_workspace_bytes(B)
        if not workspace.is_cuda or workspace.dtype != u8 or workspace.numel() < need or not workspace.is_contiguous():
            raise NativeError(f"workspace: expected a contiguous uint8 device tensor of >= {need} bytes")
    _check(load().g2048_policy_encoder(
        _dev(boards, u8, 16 * B, "boards"), _dev(embed_table, f32, 16 * 31 * 256, "embed_table"),
        _dev(cls_token, f32, 256, "cls_token"), _dev(weights_bf16, torch.bfloat16, n_layers * 786432, "weights_bf16"),
        _dev(params_f32, f32, n_layers * 3328, "params_f32"), n_layers, _dev(features, f32, 256 * B, "features"), B,
        None if workspace is None else workspace.data_ptr(), _stream()), "g2048_policy_encoder")


def policy_encoder_mean(boards, embed_table, cls_token, weights_bf16, params_f32, n_layers: int, features):
    """The "mean" reduction (mean of the 16 board tokens' outputs); same packed blobs as policy_encoder."""
    B = boards.numel() // 16
    _check(load().g2048_policy_encoder_mean(
        _dev(boards, u8, 16 * B, "boards"), _dev(embed_table, f32, 16 * 31 * 256, "embed_table"),
        _dev(cls_token, f32, 256, "cls_token"), _dev(weights_bf16, torch.bfloat16, n_layers * 786432, "weights_bf16"),
        _dev(params_f32, f32, n_layers * 3328, "params_f32"), n_layers, _dev(features, f32, 256 * B, "features"), B,
        _stream()), "g2048_policy_encoder_mean")


F32SPLIT_BIAS, F32SPLIT_BIAS_RELU = CONSTANTS["G2048_F32SPLIT_BIAS"], CONSTANTS["G2048_F32SPLIT_BIAS_RELU"]
F32SPLIT_ADD_LN, F32SPLIT_ADD = CONSTANTS["G2048_F32SPLIT_ADD_LN"], CONSTANTS["G2048_F32SPLIT_ADD"]


def f32split_pack(w, scale: float, packed):
    """w f32 [N, K] -> ``packed`` (float16, 2 N K elements): hi / lo planes of ``w * scale`` in fragment order (``g2048_f32split_pack``)."""
    N, K = w.shape
    _check(load().g2048_f32split_pack(_dev(w, f32, N * K, "w"), N, K, float(scale), _dev(packed, torch.float16, 2 * N * K, "packed"),
                                      _stream()), "g2048_f32split_pack")


def _rows(t, dtype, cols: int, name: str):
    """(data_ptr, row stride) of a 2-D device tensor with unit column stride."""
    if t is None or not t.is_cuda or t.dtype != dtype or t.dim() != 2 or t.shape[1] < cols or (t.shape[1] > 1 and t.stride(1) != 1):
        raise NativeError(f"{name}: expected a 2-D {dtype} HIP tensor with >= {cols} unit-stride columns")
    return t.data_ptr(), t.stride(0)


def f32split_gemm(x, w_packed, bias, y, K: int, N: int, epilogue: int, sx: float, sw: float, resid=None, gamma=None, beta=None, h=None,
                  eps: float = 1e-5, T=None):
    """y[:T] = epilogue(x[:T] @ W^T + bias) as a split-fp16 product (``g2048_f32split_gemm``); x, y 2-D f32 (row strides free)."""
    T = x.shape[0] if T is None else int(T)
    (xp, ldx), (yp, ldy) = _rows(x, f32, K, "x"), _rows(y, f32, N, "y")
    if x.shape[0] < T or y.shape[0] < T:
        raise NativeError("f32split_gemm: fewer than T rows")
    _check(load().g2048_f32split_gemm(
        xp, ldx, _dev(w_packed, torch.float16, 2 * N * K, "w_packed"), _dev(bias, f32, N, "bias"), yp, ldy,
        _dev(resid, f32, T * 256, "resid", optional=True), _dev(gamma, f32, 256, "gamma", optional=True),
        _dev(beta, f32, 256, "beta", optional=True), _dev(h, f32, T * 256, "h", optional=True), T, K, N, epilogue, float(sx), float(sw),
        float(eps), _stream()), "g2048_f32split_gemm")


def attn_fwd_f32(qkv, o, B: int, H: int, scale: float):
    """qkv f32 [B, 17, 96 H] -> o f32 [B, 17, 32 H] (``g2048_attn_fwd_f32``)."""
    _check(load().g2048_attn_fwd_f32(_dev(qkv, f32, B * 17 * 96 * H, "qkv"), _dev(o, f32, B * 17 * 32 * H, "o"), B, H, float(scale),
                                     _stream()), "g2048_attn_fwd_f32")


def embed_ln_f32(boards, table, cls, gamma, beta, eps: float, x0, h):
    """boards u8 [B, 16] -> x0, h = LayerNorm(x0) f32 [B, 17, 256] (``g2048_embed_ln_f32``)."""
    B = boards.numel() // 16
    _check(load().g2048_embed_ln_f32(_dev(boards, u8, 16 * B, "boards"), _dev(table, f32, 16 * 31 * 256, "table"), _dev(cls, f32, 256, "cls"),
                                     _dev(gamma, f32, 256, "gamma"), _dev(beta, f32, 256, "beta"), float(eps),
                                     _dev(x0, f32, B * 17 * 256, "x0"), _dev(h, f32, B * 17 * 256, "h"), B, _stream()),
           "g2048_embed_ln_f32")


def lookahead_expand(boards, after, reward, nchild):
    """boards u8 [B,16] -> after u8 [B,4,16], reward f32 [B,4], nchild i32 [B,4] (0 for an illegal move)."""
    B = boards.numel() // 16
    _check(load().g2048_lookahead_expand(_dev(boards, u8, 16 * B, "boards"), B, _dev(after, u8, 64 * B, "after"),
                                         _dev(reward, f32, 4 * B, "reward"), _dev(nchild, i32, 4 * B, "nchild"), _stream()),
           "g2048_lookahead_expand")


def lookahead_children(after, nchild, offset, N: int, children, terminal):
    """The N = nchild.sum() children in (b, a, cell, tile) order: children u8 [>= N,16], terminal u8 [>= N].  ``offset`` is the
    exclusive prefix sum of ``nchild``; rows past N are left alone."""
    B = nchild.numel() // 4
    N = int(N)
    if N < 0:
        raise NativeError("lookahead_children: N must not be negative")
    _check(load().g2048_lookahead_children(_dev(after, u8, 64 * B, "after"), _dev(nchild, i32, 4 * B, "nchild"),
                                           _dev(offset, i32, 4 * B, "offset"), B, N,
                                           _dev(children, u8, 16 * N, "children"), _dev(terminal, u8, N, "terminal"), _stream()),
           "g2048_lookahead_children")


def lookahead_reduce(reward, nchild, offset, values, terminal, gamma: float, N: int, q):
    """q f32 [B,4] = reward + gamma * E_spawn[V(child)], V = 0 at terminal children; 0 where nchild == 0."""
    B = nchild.numel() // 4
    N = int(N)
    if N < 0:
        raise NativeError("lookahead_reduce: N must not be negative")
    _check(load().g2048_lookahead_reduce(_dev(reward, f32, 4 * B, "reward"), _dev(nchild, i32, 4 * B, "nchild"),
                                         _dev(offset, i32, 4 * B, "offset"), _dev(values, f32, N, "values"),
                                         _dev(terminal, u8, N, "terminal"), float(gamma), B, N, _dev(q, f32, 4 * B, "q"), _stream()),
           "g2048_lookahead_reduce")


def lookahead_dedup(after, nchild, group_start, rep, nuniq):
    """Per root (pairs group_start[g] .. group_start[g + 1], at most 480): rep i32 [P] = the first pair of the group with children
    and the same afterstate bytes (itself where nchild == 0), nuniq i32 [P] = nchild at representatives, 0 elsewhere."""
    P = nchild.numel()
    G = group_start.numel() - 1
    if G < 1:
        raise NativeError("lookahead_dedup: group_start needs at least two entries")
    _check(load().g2048_lookahead_dedup(_dev(after, u8, 16 * P, "after"), _dev(nchild, i32, P, "nchild"),
                                        _dev(group_start, i32, G + 1, "group_start"), G, P, _dev(rep, i32, P, "rep"),
                                        _dev(nuniq, i32, P, "nuniq"), _stream()),
           "g2048_lookahead_dedup")


def lookahead_backup(reward, nchild, rep, e, v1):
    """v1 f32 [N1] = max over the actions with nchild > 0 of reward + e[rep] (0 where there is none); the others are [N1,4]."""
    N1 = nchild.numel() // 4
    _check(load().g2048_lookahead_backup(_dev(reward, f32, 4 * N1, "reward"), _dev(nchild, i32, 4 * N1, "nchild"),
                                         _dev(rep, i32, 4 * N1, "rep"), _dev(e, f32, 4 * N1, "e"), N1,
                                         _dev(v1, f32, N1, "v1"), _stream()),
           "g2048_lookahead_backup")


def sym_canon(boards, out_boards=None, actions=None, masks=None, frame=None, out_actions=None, out_masks=None):
    """boards u8 [B,16] -> out_boards = the canonical view of every board, frame u8 [B] = which of the 8 views it is; actions /
    masks u8 [B] (optional) turned into that view.  An output left None is written over its input (the in-place pass over a
    rollout buffer); ``frame`` left None is not written."""
    B = boards.numel() // 16
    out_boards = boards if out_boards is None else out_boards
    out_actions = actions if out_actions is None else out_actions
    out_masks = masks if out_masks is None else out_masks
    _check(load().g2048_sym_canon(_dev(boards, u8, 16 * B, "boards"), _dev(actions, u8, B, "actions", optional=True),
                                  _dev(masks, u8, B, "masks", optional=True), B, _dev(out_boards, u8, 16 * B, "out_boards"),
                                  _dev(out_actions, u8, B, "out_actions", optional=True),
                                  _dev(out_masks, u8, B, "out_masks", optional=True), _dev(frame, u8, B, "frame", optional=True),
                                  _stream()),
           "g2048_sym_canon")


def sym_logits(logits, frame, out=None):
    """logits f32 [B,4] in the canonical frame -> out[b][a] = logits[b][sigma_frame[b](a)], the env's frame (in place when
    ``out`` is None); the bit patterns are moved."""
    B = frame.numel()
    out = logits if out is None else out
    _check(load().g2048_sym_logits(_dev(logits, f32, 4 * B, "logits"), _dev(frame, u8, B, "frame"), B, _dev(out, f32, 4 * B, "out"),
                                   _stream()),
           "g2048_sym_logits")


def sym_views(boards, views):
    """boards u8 [B,16] -> views u8 [B,8,16] (or [8 B,16]): views[b][g] = view_g(boards[b]), the rows of the ensemble's forward."""
    B = boards.numel() // 16
    _check(load().g2048_sym_views(_dev(boards, u8, 16 * B, "boards"), B, _dev(views, u8, 128 * B, "views"), _stream()),
           "g2048_sym_views")


def sym_fold(logits, values, out_logits, out_values):
    """logits f32 [8 B,4] / values f32 [8 B] of a forward on ``sym_views``' rows -> out_logits f32 [B,4] / out_values f32 [B]: the
    order-free mean over the eight views, the logits in the env's frame.  Either pair may be None (both of it), not both pairs."""
    out = out_logits if out_logits is not None else out_values
    if out is None:
        raise NativeError("sym_fold: out_logits or out_values required")
    B = out.numel() // 4 if out_logits is not None else out.numel()
    _check(load().g2048_sym_fold(_dev(logits, f32, 32 * B, "logits", optional=True), _dev(values, f32, 8 * B, "values", optional=True), B,
                                 _dev(out_logits, f32, 4 * B, "out_logits", optional=True),
                                 _dev(out_values, f32, B, "out_values", optional=True), _stream()),
           "g2048_sym_fold")


def mc_playout(step_subs: np.ndarray, t0: int, roots, B: int, R: int, lane0: int, n_total: int, policy: int, gamma: float,
               lane_boards, lane_masks, lane_done, lane_ret, lane_disc, rng_mode: int, live_count=None):
    """``len(step_subs)`` playout steps (global steps t0 ..) of the 4 B R lanes of B roots, R playouts per (board, action) pair.
    step_subs u32 [n_steps, 4] (host): act sub-key, step sub-key.  t0 == 0 seeds the lanes from roots u8 [B,16]; t0 > 0 continues
    from the lane arrays (roots may be None).  live_count: i32 [1] zeroed by the caller, or None."""
    subs = np.ascontiguousarray(step_subs, np.uint32).reshape(-1, 4)
    B, R = int(B), int(R)
    n = 4 * B * R
    _check(load().g2048_mc_playout(subs.ctypes.data, subs.shape[0], int(t0), _dev(roots, u8, 16 * B, "roots", optional=t0 > 0), B, R,
                                   int(lane0), int(n_total), int(policy), float(gamma), _dev(lane_boards, u8, 16 * n, "lane_boards"),
                                   _dev(lane_masks, u8, n, "lane_masks"), _dev(lane_done, u8, n, "lane_done"),
                                   _dev(lane_ret, f32, n, "lane_ret"), _dev(lane_disc, f32, n, "lane_disc"), int(rng_mode),
                                   _dev(live_count, i32, 1, "live_count", optional=True), _stream()),
           "g2048_mc_playout")


def mc_reduce(lane_ret, lane_disc, lane_done, leaf_values, R: int, q):
    """q f32 [B,4] = the mean over each pair's R lanes of ret (+ disc * leaf_values where the lane is alive and leaf_values f32
    [4 B R] is given), summed in ascending lane order."""
    B, R = q.numel() // 4, int(R)
    n = 4 * B * R
    _check(load().g2048_mc_reduce(_dev(lane_ret, f32, n, "lane_ret"), _dev(lane_disc, f32, n, "lane_disc"),
                                  _dev(lane_done, u8, n, "lane_done"), _dev(leaf_values, f32, n, "leaf_values", optional=True), B, R,
                                  _dev(q, f32, 4 * B, "q"), _stream()),
           "g2048_mc_reduce")


def _tuple_cells(tuple_cells):
    """tuple_cells u8 [m, L] (host) -> (contiguous array, m, L)."""
    cells = np.ascontiguousarray(tuple_cells, np.uint8)
    if cells.ndim != 2:
        raise NativeError(f"tuple_cells: expected a [m, L] array of cell indices, got shape {cells.shape}")
    return cells, cells.shape[0], cells.shape[1]


def _stages(stage_tiles):
    """stage_tiles, the ascending log2 tile thresholds (host) -> (contiguous u8 array, n_stages = their number + 1)."""
    st = np.ascontiguousarray(stage_tiles, np.uint8)
    if st.ndim != 1:
        raise NativeError(f"stage_tiles: expected a flat sequence of log2 tile values, got shape {st.shape}")
    return st, st.size + 1


def ntuple_values(boards, weights, tuple_cells, frac_bits: int, values, stage_tiles=None):
    """values f32 [n] = V(boards u8 [n,16]) of the n-tuple network ``weights`` i32 [m, 16^L] over ``tuple_cells`` u8 [m, L] (host).
    ``stage_tiles`` (here and below): None, or the thresholds of a multi-stage network (host), whose tables are [S, m, 16^L]."""
    cells, m, L = _tuple_cells(tuple_cells)
    n = values.numel()
    if stage_tiles is None:
        _check(load().g2048_ntuple_values(_dev(boards, u8, 16 * n, "boards"), n, _dev(weights, i32, m * 16 ** L, "weights"),
                                          cells.ctypes.data, m, L, int(frac_bits), _dev(values, f32, n, "values"), _stream()),
               "g2048_ntuple_values")
        return
    st, S = _stages(stage_tiles)
    _check(load().g2048_ntuple_staged_values(_dev(boards, u8, 16 * n, "boards"), n, _dev(weights, i32, S * m * 16 ** L, "weights"),
                                             cells.ctypes.data, m, L, st.ctypes.data, S, int(frac_bits),
                                             _dev(values, f32, n, "values"), _stream()),
           "g2048_ntuple_staged_values")


def ntuple_scores(boards, weights, tuple_cells, frac_bits: int, scores, values, stage_tiles=None):
    """scores f32 [B,4] = reward + V(afterstate) per action (+0 where illegal), values f32 [B] = the max over the legal ones."""
    cells, m, L = _tuple_cells(tuple_cells)
    B = values.numel()
    if stage_tiles is None:
        _check(load().g2048_ntuple_scores(_dev(boards, u8, 16 * B, "boards"), B, _dev(weights, i32, m * 16 ** L, "weights"),
                                          cells.ctypes.data, m, L, int(frac_bits), _dev(scores, f32, 4 * B, "scores"),
                                          _dev(values, f32, B, "values"), _stream()),
               "g2048_ntuple_scores")
        return
    st, S = _stages(stage_tiles)
    _check(load().g2048_ntuple_staged_scores(_dev(boards, u8, 16 * B, "boards"), B, _dev(weights, i32, S * m * 16 ** L, "weights"),
                                             cells.ctypes.data, m, L, st.ctypes.data, S, int(frac_bits),
                                             _dev(scores, f32, 4 * B, "scores"), _dev(values, f32, B, "values"), _stream()),
           "g2048_ntuple_staged_scores")


def ntuple_expectimax_workspace_floats(B: int, plies: int) -> int:
    """The f32 elements of ``workspace`` that ``ntuple_expectimax`` needs: 0 for one ply, 128 B for two."""
    n = load().g2048_ntuple_expectimax_workspace_floats(int(B), int(plies))
    if n < 0:
        raise NativeError(f"ntuple_expectimax: no workspace size for B={B}, plies={plies} (plies is 1 or 2, B at most 2^24 / 2^20)")
    return n


def ntuple_expectimax(boards, weights, tuple_cells, frac_bits: int, plies: int, gamma: float, workspace, scores, values,
                      stage_tiles=None):
    """scores f32 [B,4] = the ``plies``-ply (1 or 2) expectimax Q over the n-tuple network's greedy value, values f32 [B] = the max
    over the legal moves.  workspace: f32 [>= 128 B] for two plies, None (or anything) for one; its contents do not matter."""
    cells, m, L = _tuple_cells(tuple_cells)
    B, plies = values.numel(), int(plies)
    need = ntuple_expectimax_workspace_floats(B, plies)
    if stage_tiles is None:
        _check(load().g2048_ntuple_expectimax(_dev(boards, u8, 16 * B, "boards"), B, _dev(weights, i32, m * 16 ** L, "weights"),
                                              cells.ctypes.data, m, L, int(frac_bits), plies, float(gamma),
                                              _dev(workspace, f32, need, "workspace", optional=need == 0),
                                              _dev(scores, f32, 4 * B, "scores"), _dev(values, f32, B, "values"), _stream()),
               "g2048_ntuple_expectimax")
        return
    st, S = _stages(stage_tiles)
    _check(load().g2048_ntuple_staged_expectimax(_dev(boards, u8, 16 * B, "boards"), B,
                                                 _dev(weights, i32, S * m * 16 ** L, "weights"), cells.ctypes.data, m, L,
                                                 st.ctypes.data, S, int(frac_bits), plies, float(gamma),
                                                 _dev(workspace, f32, need, "workspace", optional=need == 0),
                                                 _dev(scores, f32, 4 * B, "scores"), _dev(values, f32, B, "values"), _stream()),
           "g2048_ntuple_staged_expectimax")


def ntuple_search_workspace_bytes(B: int, depth: int) -> int:
    """The bytes of ``workspace`` that ``ntuple_search`` needs for B roots at ``depth`` (the worst case: no list can overflow)."""
    n = load().g2048_ntuple_search_workspace_bytes(int(B), int(depth))
    if n < 0:
        raise NativeError(f"ntuple_search: no workspace size for B={B}, depth={depth} (depth is 1, 2 or 3, B at most 2^20 / 2^16 / 2^12)")
    return n


def ntuple_search(boards, weights, tuple_cells, frac_bits: int, depth: int, gamma: float, dedup: bool, workspace, scores, values,
                  counts=None, stage_tiles=None):
    """scores f32 [B,4] = the ``depth``-ply (1, 2 or 3) expectimax Q over the n-tuple network's greedy value, searched on packed lists
    of afterstates (``dedup``: the equal afterstates of one root merged), values f32 [B] = the max over the legal moves.  workspace:
    uint8 [>= ntuple_search_workspace_bytes(B, depth)], its contents do not matter; counts: i32 [3] or None, the entries per level."""
    cells, m, L = _tuple_cells(tuple_cells)
    B, depth = values.numel(), int(depth)
    need = ntuple_search_workspace_bytes(B, depth)
    st, S = (None, 1) if stage_tiles is None else _stages(stage_tiles)
    args = (_dev(boards, u8, 16 * B, "boards"), B, _dev(weights, i32, S * m * 16 ** L, "weights"), cells.ctypes.data, m, L)
    tail = (int(frac_bits), depth, float(gamma), int(bool(dedup)), _dev(workspace, u8, need, "workspace"), workspace.numel(),
            _dev(scores, f32, 4 * B, "scores"), _dev(values, f32, B, "values"), _dev(counts, i32, 3, "counts", optional=True), _stream())
    if stage_tiles is None:
        _check(load().g2048_ntuple_search(*args, *tail), "g2048_ntuple_search")
    else:
        _check(load().g2048_ntuple_staged_search(*args, st.ctypes.data, S, *tail), "g2048_ntuple_staged_search")


def ntuple_budget_search_workspace_bytes(B: int, max_depth: int, budget: int) -> int:
    """The bytes of ``workspace`` that ``ntuple_budget_search`` needs for B roots: every root owns a region per level."""
    n = load().g2048_ntuple_budget_search_workspace_bytes(int(B), int(max_depth), int(budget))
    if n < 0:
        raise NativeError(f"ntuple_budget_search: no workspace size for B={B}, max_depth={max_depth}, budget={budget} (max_depth is "
                          f"1 .. 6, budget 4 .. 24576, B at most min(2^20, (2^31 - 1) // (128 * the largest region's entries)))")
    return n


def ntuple_budget_search(boards, weights, tuple_cells, frac_bits: int, max_depth: int, budget: int, gamma: float, workspace, scores,
                         values, depth_used=None, entries=None, stage_tiles=None):
    """scores f32 [B,4] = the expectimax Q over the n-tuple network's greedy value, every root searched as deep (1 .. ``max_depth``) as
    its levels hold at most ``budget`` distinct afterstates; values f32 [B] = the max over the legal moves.  workspace: uint8 [>=
    ntuple_budget_search_workspace_bytes(B, max_depth, budget)], its contents do not matter; depth_used: u8 [B] or None, the depth of
    every root; entries: i32 [B, 6] or None, its distinct afterstates per level."""
    cells, m, L = _tuple_cells(tuple_cells)
    B, max_depth, budget = values.numel(), int(max_depth), int(budget)
    need = ntuple_budget_search_workspace_bytes(B, max_depth, budget)
    st, S = (None, 1) if stage_tiles is None else _stages(stage_tiles)
    args = (_dev(boards, u8, 16 * B, "boards"), B, _dev(weights, i32, S * m * 16 ** L, "weights"), cells.ctypes.data, m, L)
    tail = (int(frac_bits), max_depth, budget, float(gamma), _dev(workspace, u8, need, "workspace"), workspace.numel(),
            _dev(scores, f32, 4 * B, "scores"), _dev(values, f32, B, "values"), _dev(depth_used, u8, B, "depth_used", optional=True),
            _dev(entries, i32, 6 * B, "entries", optional=True), _stream())
    if stage_tiles is None:
        _check(load().g2048_ntuple_budget_search(*args, *tail), "g2048_ntuple_budget_search")
    else:
        _check(load().g2048_ntuple_staged_budget_search(*args, st.ctypes.data, S, *tail), "g2048_ntuple_staged_budget_search")


def ntuple_td_accumulate(prev_after, flag, target, weights, tuple_cells, frac_bits: int, alpha: float, acc, cnt, td_error=None,
                         stage_tiles=None):
    """The accumulate half of one TD(0) lock-step: acc i64 [m, 16^L] += delta, cnt i32 [m, 16^L] += 1 at the entries of every env
    with flag != 0.  td_error f32 [B] or None."""
    cells, m, L = _tuple_cells(tuple_cells)
    B, E = flag.numel(), m * 16 ** L
    if stage_tiles is None:
        _check(load().g2048_ntuple_td_accumulate(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"),
                                                 _dev(target, f32, B, "target"), B, _dev(weights, i32, E, "weights"),
                                                 cells.ctypes.data, m, L, int(frac_bits), float(alpha), _dev(acc, i64, E, "acc"),
                                                 _dev(cnt, i32, E, "cnt"), _dev(td_error, f32, B, "td_error", optional=True),
                                                 _stream()),
               "g2048_ntuple_td_accumulate")
        return
    st, S = _stages(stage_tiles)
    E *= S
    _check(load().g2048_ntuple_staged_td_accumulate(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"),
                                                    _dev(target, f32, B, "target"), B, _dev(weights, i32, E, "weights"),
                                                    cells.ctypes.data, m, L, st.ctypes.data, S, int(frac_bits), float(alpha),
                                                    _dev(acc, i64, E, "acc"), _dev(cnt, i32, E, "cnt"),
                                                    _dev(td_error, f32, B, "td_error", optional=True), _stream()),
           "g2048_ntuple_staged_td_accumulate")


def ntuple_td_apply(prev_after, flag, tuple_cells, weights, acc, cnt, stage_tiles=None):
    """The apply half: weights += the rounded mean acc / cnt at every entry the same boards hit, acc = cnt = 0 there."""
    cells, m, L = _tuple_cells(tuple_cells)
    B, E = flag.numel(), m * 16 ** L
    if stage_tiles is None:
        _check(load().g2048_ntuple_td_apply(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"), B,
                                            cells.ctypes.data, m, L, _dev(weights, i32, E, "weights"), _dev(acc, i64, E, "acc"),
                                            _dev(cnt, i32, E, "cnt"), _stream()),
               "g2048_ntuple_td_apply")
        return
    st, S = _stages(stage_tiles)
    E *= S
    _check(load().g2048_ntuple_staged_td_apply(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"), B,
                                               cells.ctypes.data, m, L, st.ctypes.data, S, _dev(weights, i32, E, "weights"),
                                               _dev(acc, i64, E, "acc"), _dev(cnt, i32, E, "cnt"), _stream()),
           "g2048_ntuple_staged_td_apply")


def ntuple_tc_accumulate(prev_after, flag, target, weights, tuple_cells, frac_bits: int, alpha: float, acc, abs_acc, cnt,
                         td_error=None, stage_tiles=None):
    """The accumulate half of one TC lock-step: acc i64 [m, 16^L] += delta, abs_acc i64 [m, 16^L] += |delta|, cnt i32 [m, 16^L] += 1
    at the entries of every env with flag != 0.  td_error f32 [B] or None."""
    cells, m, L = _tuple_cells(tuple_cells)
    B, E = flag.numel(), m * 16 ** L
    if stage_tiles is None:
        _check(load().g2048_ntuple_tc_accumulate(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"),
                                                 _dev(target, f32, B, "target"), B, _dev(weights, i32, E, "weights"),
                                                 cells.ctypes.data, m, L, int(frac_bits), float(alpha), _dev(acc, i64, E, "acc"),
                                                 _dev(abs_acc, i64, E, "abs_acc"), _dev(cnt, i32, E, "cnt"),
                                                 _dev(td_error, f32, B, "td_error", optional=True), _stream()),
               "g2048_ntuple_tc_accumulate")
        return
    st, S = _stages(stage_tiles)
    E *= S
    _check(load().g2048_ntuple_staged_tc_accumulate(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"),
                                                    _dev(target, f32, B, "target"), B, _dev(weights, i32, E, "weights"),
                                                    cells.ctypes.data, m, L, st.ctypes.data, S, int(frac_bits), float(alpha),
                                                    _dev(acc, i64, E, "acc"), _dev(abs_acc, i64, E, "abs_acc"),
                                                    _dev(cnt, i32, E, "cnt"), _dev(td_error, f32, B, "td_error", optional=True),
                                                    _stream()),
           "g2048_ntuple_staged_tc_accumulate")


def ntuple_tc_apply(prev_after, flag, tuple_cells, weights, acc, abs_acc, cnt, coh_e, coh_a, stage_tiles=None):
    """The apply half: every entry the same boards hit moves by its rounded mean delta times its rate |coh_e| / coh_a (rate 1
    where coh_a == 0), coh_e += the mean, coh_a += the mean magnitude, acc = abs_acc = cnt = 0 there."""
    cells, m, L = _tuple_cells(tuple_cells)
    B, E = flag.numel(), m * 16 ** L
    if stage_tiles is None:
        _check(load().g2048_ntuple_tc_apply(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"), B,
                                            cells.ctypes.data, m, L, _dev(weights, i32, E, "weights"), _dev(acc, i64, E, "acc"),
                                            _dev(abs_acc, i64, E, "abs_acc"), _dev(cnt, i32, E, "cnt"), _dev(coh_e, i32, E, "coh_e"),
                                            _dev(coh_a, i32, E, "coh_a"), _stream()),
               "g2048_ntuple_tc_apply")
        return
    st, S = _stages(stage_tiles)
    E *= S
    _check(load().g2048_ntuple_staged_tc_apply(_dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"), B,
                                               cells.ctypes.data, m, L, st.ctypes.data, S, _dev(weights, i32, E, "weights"),
                                               _dev(acc, i64, E, "acc"), _dev(abs_acc, i64, E, "abs_acc"), _dev(cnt, i32, E, "cnt"),
                                               _dev(coh_e, i32, E, "coh_e"), _dev(coh_a, i32, E, "coh_a"), _stream()),
           "g2048_ntuple_staged_tc_apply")


def ntuple_link(tr_boards_row, tr_meta_row, prev_after, flag):
    """prev_after u8 [B,16] = the afterstate of the move recorded in one trajectory row, flag u8 [B] = 2 where it ended the episode."""
    B = flag.numel()
    _check(load().g2048_ntuple_link(_dev(tr_boards_row, u8, 16 * B, "tr_boards_row"), _dev(tr_meta_row, u8, B, "tr_meta_row"), B,
                                    _dev(prev_after, u8, 16 * B, "prev_after"), _dev(flag, u8, B, "flag"), _stream()),
           "g2048_ntuple_link")


def _exact(t, dtype, shape, name: str, optional=False):
    """``_dev`` plus the exact shape."""
    if t is not None and tuple(t.shape) != tuple(shape):
        raise NativeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return _dev(t, dtype, None, name, optional)


def ntuple_carousel_record(boards, masks, flag, carousel_tiles, reached, pool_boards, pool_masks):
    """The record half of the carousel: every env with flag == 1 whose board u8 [B,16] has entered carousel stage s > reached u8 [B]
    puts board and mask into slot (s - 1, b) of pool_boards u8 [n,B,16] / pool_masks u8 [n,B], reached = s.  ``carousel_tiles``:
    the n ascending log2 tile thresholds (host)."""
    st, S = _stages(carousel_tiles)
    n, B = S - 1, flag.numel()
    _check(load().g2048_ntuple_carousel_record(_exact(boards, u8, (B, 16), "boards"), _exact(masks, u8, (B,), "masks"),
                                               _exact(flag, u8, (B,), "flag"), B, st.ctypes.data, n,
                                               _exact(reached, u8, (B,), "reached"), _exact(pool_boards, u8, (n, B, 16), "pool_boards"),
                                               _exact(pool_masks, u8, (n, B), "pool_masks"), _stream()),
           "g2048_ntuple_carousel_record")


def ntuple_carousel_restart(sub, flag, pool_boards, pool_masks, boards, masks, reached, turn, starts, rng_mode: int, start_stage=None):
    """The restart half: every env with flag == 2 takes its turn (turn i32 [B], the bits of a u32) and starts its episode at a donor's
    pool board of the turn's stage if there is one, else at the fresh board it holds; starts i64 [n + 1] counts per stage.  ``sub``:
    the lock-step's act sub-key (host u32 [2]).  start_stage u8 [B] or None: the stage per restarted env, 0xFF elsewhere."""
    B = flag.numel()
    n = pool_masks.shape[0] if pool_masks is not None and pool_masks.dim() == 2 else 0
    _check(load().g2048_ntuple_carousel_restart(int(sub[0]), int(sub[1]), _exact(flag, u8, (B,), "flag"), B, n,
                                                _exact(pool_boards, u8, (n, B, 16), "pool_boards"),
                                                _exact(pool_masks, u8, (n, B), "pool_masks"), _exact(boards, u8, (B, 16), "boards"),
                                                _exact(masks, u8, (B,), "masks"), _exact(reached, u8, (B,), "reached"),
                                                _exact(turn, KEY_DTYPE, (B,), "turn"), _exact(starts, i64, (n + 1,), "starts"),
                                                _exact(start_stage, u8, (B,), "start_stage", optional=True), int(rng_mode), _stream()),
           "g2048_ntuple_carousel_restart")


def _ring(hist, hist_len, B: int):
    """The delayed learner's ring: hist u8 [h, B, 16], hist_len u8 [B] -> (hist pointer, hist_len pointer, h)."""
    h = hist.shape[0] if hist is not None and hist.dim() == 3 else 0
    return _exact(hist, u8, (h, B, 16), "hist"), _exact(hist_len, u8, (B,), "hist_len"), h


def ntuple_delayed_accumulate(hist, hist_err, hist_len, flag, target, head: int, lam: float, weights, tuple_cells, frac_bits: int,
                              alpha: float, acc, abs_acc, cnt, td_error=None, stage_tiles=None):
    """The accumulate half of one delayed TD(lambda) / TC(lambda) lock-step over the ring hist u8 [h, B, 16] / hist_err f32 [h, B] /
    hist_len u8 [B] whose newest afterstate is in slot ``head``: e of that afterstate -> td_error and hist_err[head]; acc += delta_j,
    cnt += 1 (abs_acc += |delta_j| unless ``abs_acc`` is None: TD) at the entries of every DUE state of every env with flag != 0,
    delta_j from the lambda-sum of the errors since.  The tables are [m, 16^L], or [S, m, 16^L] with ``stage_tiles``."""
    cells, m, L = _tuple_cells(tuple_cells)
    B = flag.numel()
    st, S = (None, 1) if stage_tiles is None else _stages(stage_tiles)
    E = S * m * 16 ** L
    p_hist, p_len, h = _ring(hist, hist_len, B)
    _check(load().g2048_ntuple_delayed_accumulate(p_hist, _exact(hist_err, f32, (h, B), "hist_err"), p_len, _exact(flag, u8, (B,), "flag"),
                                                  _dev(target, f32, B, "target"), B, h, int(head), float(lam),
                                                  _dev(weights, i32, E, "weights"), cells.ctypes.data, m, L,
                                                  None if st is None else st.ctypes.data, S, int(frac_bits), float(alpha),
                                                  _dev(acc, i64, E, "acc"), _dev(abs_acc, i64, E, "abs_acc", optional=True),
                                                  _dev(cnt, i32, E, "cnt"), _dev(td_error, f32, B, "td_error", optional=True), _stream()),
           "g2048_ntuple_delayed_accumulate")


def ntuple_delayed_apply(hist, hist_len, flag, head: int, tuple_cells, weights, acc, abs_acc, cnt, coh_e, coh_a, stage_tiles=None):
    """The apply half over the same due states: td_apply per due board with ``abs_acc``, ``coh_e`` and ``coh_a`` all None, tc_apply with
    none of them None."""
    cells, m, L = _tuple_cells(tuple_cells)
    B = flag.numel()
    st, S = (None, 1) if stage_tiles is None else _stages(stage_tiles)
    E = S * m * 16 ** L
    p_hist, p_len, h = _ring(hist, hist_len, B)
    _check(load().g2048_ntuple_delayed_apply(p_hist, p_len, _exact(flag, u8, (B,), "flag"), B, h, int(head), cells.ctypes.data, m, L,
                                             None if st is None else st.ctypes.data, S, _dev(weights, i32, E, "weights"),
                                             _dev(acc, i64, E, "acc"), _dev(abs_acc, i64, E, "abs_acc", optional=True),
                                             _dev(cnt, i32, E, "cnt"), _dev(coh_e, i32, E, "coh_e", optional=True),
                                             _dev(coh_a, i32, E, "coh_a", optional=True), _stream()),
           "g2048_ntuple_delayed_apply")


def ntuple_delayed_link(tr_boards_row, tr_meta_row, slot: int, prev_after, flag, hist, hist_len):
    """``ntuple_link`` for the delayed learner: the new afterstate goes to prev_after u8 [B,16] and to hist[slot], hist_len u8 [B]
    grows by one up to h and restarts at 1 after an episode end (the old flag == 2)."""
    B = flag.numel()
    p_hist, p_len, h = _ring(hist, hist_len, B)
    _check(load().g2048_ntuple_delayed_link(_dev(tr_boards_row, u8, 16 * B, "tr_boards_row"), _dev(tr_meta_row, u8, B, "tr_meta_row"), B,
                                            h, int(slot), _exact(prev_after, u8, (B, 16), "prev_after"), _exact(flag, u8, (B,), "flag"),
                                            p_hist, p_len, _stream()),
           "g2048_ntuple_delayed_link")


def ntuple_episodes(start: bool, n_steps: int, bs: int, weights, tuple_cells, frac_bits: int, chain, boards, masks, done, ep_len, score,
                    rng_mode: int, live_count=None, stage_tiles=None):
    """``n_steps`` greedy steps of the N = ``done.numel()`` games of an evaluation in batches of ``bs``, every game in a quad of one
    persistent launch.  chain i32 [N,2] (the u32 key words): with ``start`` the key of each game's batch, from which the games are
    seeded and boards u8 [N,16], masks u8 [N], done u8 [N], ep_len i32 [N], score i64 [N] are output only; without it all six
    continue.  live_count: i32 [1] zeroed by the caller, or None."""
    cells, m, L = _tuple_cells(tuple_cells)
    N = done.numel()
    st, S = (None, 1) if stage_tiles is None else _stages(stage_tiles)
    head = (int(bool(start)), int(n_steps), N, int(bs), _dev(weights, i32, S * m * 16 ** L, "weights"), cells.ctypes.data, m, L)
    tail = (int(frac_bits), _exact(chain, KEY_DTYPE, (N, 2), "chain"), _exact(boards, u8, (N, 16), "boards"),
            _exact(masks, u8, (N,), "masks"), _exact(done, u8, (N,), "done"), _exact(ep_len, i32, (N,), "ep_len"),
            _exact(score, i64, (N,), "score"), int(rng_mode), _dev(live_count, i32, 1, "live_count", optional=True), _stream())
    if stage_tiles is None:
        _check(load().g2048_ntuple_episodes(*head, *tail), "g2048_ntuple_episodes")
    else:
        _check(load().g2048_ntuple_staged_episodes(*head, st.ctypes.data, S, *tail), "g2048_ntuple_staged_episodes")


def ntuple_search_episodes(start: bool, n_steps: int, bs: int, weights, tuple_cells, frac_bits: int, plies: int, gamma: float, chain,
                           boards, masks, done, ep_len, score, rng_mode: int, live_count=None, stage_tiles=None):
    """``ntuple_episodes`` with every move chosen by ``plies`` (1) plies of expectimax at discount ``gamma``, one wavefront per game.
    The operands and the launch semantics are ``ntuple_episodes``'s."""
    cells, m, L = _tuple_cells(tuple_cells)
    N = done.numel()
    st, S = (None, 1) if stage_tiles is None else _stages(stage_tiles)
    head = (int(bool(start)), int(n_steps), N, int(bs), _dev(weights, i32, S * m * 16 ** L, "weights"), cells.ctypes.data, m, L)
    tail = (int(frac_bits), int(plies), float(gamma), _exact(chain, KEY_DTYPE, (N, 2), "chain"), _exact(boards, u8, (N, 16), "boards"),
            _exact(masks, u8, (N,), "masks"), _exact(done, u8, (N,), "done"), _exact(ep_len, i32, (N,), "ep_len"),
            _exact(score, i64, (N,), "score"), int(rng_mode), _dev(live_count, i32, 1, "live_count", optional=True), _stream())
    if stage_tiles is None:
        _check(load().g2048_ntuple_search_episodes(*head, *tail), "g2048_ntuple_search_episodes")
    else:
        _check(load().g2048_ntuple_staged_search_episodes(*head, st.ctypes.data, S, *tail), "g2048_ntuple_staged_search_episodes")


def attn_fwd(q_ptr: int, k_ptr: int, v_ptr: int, o, lse, B: int, H: int, Sq: int, strides, scale: float, p_drop: float,
             seed: int, seed_state: int = 0):
    """q/k/v: raw device addresses inside bf16 tensors the caller keeps alive; strides = (q_sb, q_ss, k_sb, k_ss,
    v_sb, v_ss) in elements."""
    _check(load().g2048_attn_fwd(q_ptr, k_ptr, v_ptr, _dev(o, torch.bfloat16, B * Sq * H * 32, "o"),
                                 _dev(lse, f32, B * H * Sq, "lse"), B, H, Sq, *[int(x) for x in strides], float(scale),
                                 float(p_drop), int(seed), seed_state or None, _stream()), "g2048_attn_fwd")


def attn_bwd(q_ptr: int, k_ptr: int, v_ptr: int, dout, lse, dq_ptr: int, dk_ptr: int, dv_ptr: int, B: int, H: int,
             Sq: int, strides, scale: float, p_drop: float, seed: int, seed_state: int = 0):
    _check(load().g2048_attn_bwd(q_ptr, k_ptr, v_ptr, _dev(dout, torch.bfloat16, B * Sq * H * 32, "dout"),
                                 _dev(lse, f32, B * H * Sq, "lse"), dq_ptr, dk_ptr, dv_ptr, B, H, Sq,
                                 *[int(x) for x in strides], float(scale), float(p_drop), int(seed), seed_state or None,
                                 _stream()), "g2048_attn_bwd")


def add_ln_fwd(x_ptr: int, x_row_stride: int, a, gamma, beta, x_new, h, mean, rstd, T: int, eps: float, p_drop: float,
               seed: int, seed_state: int = 0):
    """x_ptr: raw device address of f32 rows (stride x_row_stride elements) the caller keeps alive.  gamma None: no
    LayerNorm, h = bf16(x + dropout(a)); beta, mean, rstd, x_new may then be None."""
    bf = torch.bfloat16
    _check(load().g2048_add_ln_fwd(x_ptr, int(x_row_stride), _dev(a, bf, 256 * T, "a", optional=True),
                                   _dev(gamma, f32, 256, "gamma", optional=True), _dev(beta, f32, 256, "beta", optional=True),
                                   _dev(x_new, f32, 256 * T, "x_new", optional=True), _dev(h, bf, 256 * T, "h"),
                                   _dev(mean, f32, T, "mean", optional=True), _dev(rstd, f32, T, "rstd", optional=True), T,
                                   float(eps), float(p_drop),
                                   int(seed), seed_state or None, _stream()), "g2048_add_ln_fwd")


def add_ln_bwd(xn_ptr: int, x_row_stride: int, g_x, g_h, mean, rstd, gamma, dx, da, dparams, T: int,
               p_drop: float, seed: int, seed_state: int = 0, g_x_period: int = 1):
    """dparams f32 [3, 256]: dgamma, dbeta, column sums of da.  dparams None: first stage only -> the workspace, f32
    [rows, 768] partial sums (for ``reduce_jobs``).  gamma None: the forward had no LayerNorm (xn_ptr 0, mean/rstd None)."""
    bf = torch.bfloat16
    ws = torch.empty(load().g2048_add_ln_bwd_workspace_floats(T), dtype=f32, device=dx.device)
    _check(load().g2048_add_ln_bwd(xn_ptr, int(x_row_stride), _dev(g_x, f32, 256 * (T // g_x_period), "g_x", optional=True),
                                   _dev(g_h, bf, 256 * T, "g_h"), _dev(mean, f32, T, "mean", optional=True),
                                   _dev(rstd, f32, T, "rstd", optional=True), _dev(gamma, f32, 256, "gamma", optional=True),
                                   _dev(dx, f32, 256 * T, "dx"),
                                   _dev(da, bf, 256 * T, "da", optional=True), _dev(dparams, f32, 768, "dparams", optional=True),
                                   ws.data_ptr(), T, float(p_drop), int(seed), seed_state or None, int(g_x_period), _stream()),
           "g2048_add_ln_bwd")
    return ws.view(-1, 768) if dparams is None else None


def rowgemm_ok(u2: torch.Tensor, w_packed: torch.Tensor, tile_stride: int = 0) -> bool:
    """Operands ``g2048_linear_add_ln_fwd / _bwd`` take: u2 bf16 [T, K] with unit column stride, K a multiple of 256, the packed weight
    a flat bf16 tensor of 256 * K elements - or, with ``tile_stride`` (elements between the 32-row tiles of a WIDER packed matrix), a
    flat view that starts at the first of K / 16 consecutive k-steps of it."""
    if u2.dim() != 2 or not u2.is_cuda or u2.dtype != torch.bfloat16 or u2.stride(1) != 1:
        return False
    T, K = u2.shape
    span = 256 * K if not tile_stride else 7 * int(tile_stride) + (K // 16) * 512
    return (T > 0 and K % 256 == 0 and 256 <= K <= 1024 and u2.stride(0) >= K and u2.stride(0) % 8 == 0 and u2.data_ptr() % 16 == 0
            and w_packed is not None and w_packed.is_cuda and w_packed.dtype == torch.bfloat16 and w_packed.is_contiguous()
            and (w_packed.numel() == span if not tile_stride else (w_packed.numel() >= span and tile_stride >= (K // 16) * 512
                                                                  and tile_stride % 8 == 0))
            and w_packed.data_ptr() % 16 == 0 and 160 * u2.stride(0) * 2 < 2 ** 31)


def linear_add_ln_fwd(u2, w_packed, bias, x_ptr: int, x_row_stride: int, gamma, beta, x_new, h, mean, rstd, eps: float,
                      p_drop: float, seed: int, seed_state: int = 0):
    """x_new = x + dropout(u2 W^T + bias); h = bf16(LayerNorm(x_new)) in one launch (``g2048_linear_add_ln_fwd``).  u2 bf16 [T, K];
    w_packed: fragment-packed bf16 [256][K] (``pack_fragments``); x_ptr: raw address of the f32 residual rows (stride in elements)."""
    if not rowgemm_ok(u2, w_packed):
        raise NativeError(f"linear_add_ln_fwd: operands {tuple(u2.shape)} (strides {u2.stride()}) x packed {w_packed.numel()} not supported")
    T, K = u2.shape
    bf = torch.bfloat16
    _check(load().g2048_linear_add_ln_fwd(u2.data_ptr(), u2.stride(0), w_packed.data_ptr(), _dev(bias, f32, 256, "bias", optional=True),
                                          K, x_ptr, int(x_row_stride), _dev(gamma, f32, 256, "gamma"), _dev(beta, f32, 256, "beta"),
                                          _dev(x_new, f32, 256 * T, "x_new"), _dev(h, bf, 256 * T, "h"), _dev(mean, f32, T, "mean"),
                                          _dev(rstd, f32, T, "rstd"), T, float(eps), float(p_drop), int(seed), seed_state or None,
                                          _stream()), "g2048_linear_add_ln_fwd")


def linear_add_ln_bwd(dy2, wt_packed, xn_ptr: int, x_row_stride: int, g_x, mean, rstd, gamma, dx, da, p_drop: float, seed: int,
                      seed_state: int = 0, g_x_period: int = 1, tile_stride: int = 0, g_h_extra=None, extra_period: int = 1):
    """g_h = bf16(dy2 Wt^T) and the add+LayerNorm backward on it in one launch (``g2048_linear_add_ln_bwd``) -> f32 [rows, 768] partial
    sums (dgamma | dbeta | column sums of da) for ``reduce_jobs``.  wt_packed: the fragment-packed TRANSPOSE [256][K] of the weight of
    the Linear that consumed h (``tile_stride``: see ``rowgemm_ok``).  ``g_h_extra`` bf16 [T / extra_period, 256]: added to g_h on the
    rows tok % extra_period == 0."""
    if not rowgemm_ok(dy2, wt_packed, tile_stride):
        raise NativeError(f"linear_add_ln_bwd: operands {tuple(dy2.shape)} (strides {dy2.stride()}) x packed {wt_packed.numel()} not supported")
    T, K = dy2.shape
    bf = torch.bfloat16
    ws = torch.empty((int(load().g2048_linear_add_ln_bwd_partial_rows(T)), 768), dtype=f32, device=dx.device)
    _check(load().g2048_linear_add_ln_bwd(dy2.data_ptr(), dy2.stride(0), wt_packed.data_ptr(), int(tile_stride), K, xn_ptr,
                                          int(x_row_stride), _dev(g_x, f32, 256 * (T // g_x_period), "g_x", optional=True),
                                          int(g_x_period),
                                          _dev(g_h_extra, bf, 256 * (T // max(int(extra_period), 1)), "g_h_extra", optional=True),
                                          int(extra_period), _dev(mean, f32, T, "mean"), _dev(rstd, f32, T, "rstd"), _dev(gamma, f32, 256, "gamma"),
                                          _dev(dx, f32, 256 * T, "dx"), _dev(da, bf, 256 * T, "da", optional=True), ws.data_ptr(), T,
                                          float(p_drop), int(seed), seed_state or None, _stream()), "g2048_linear_add_ln_bwd")
    return ws


# ---- MLP policy (configs[1]): csrc/g2048_mlp.hip ---------------------------------------------------------------------------------
GEMM_MAX_JOBS = CONSTANTS["G2048_GEMM_MAX_JOBS"]
GemmJob = STRUCTS["g2048_gemm_job"]


def _bf16_rows(t: torch.Tensor, name: str):
    if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16:
        raise NativeError(f"{name}: expected a bf16 [rows, cols] device tensor with unit column stride, 16-byte aligned rows; got "
                          f"{tuple(t.shape)} {t.dtype} strides {t.stride()}")
    return t.data_ptr(), t.stride(0)


def gemm_jobs(jobs, M: int):
    """``g2048_gemm_jobs``: jobs = list of dicts ``segs`` [(x [M, k] bf16, w [N, k] bf16), ...] (one or two), ``y`` [M, N] bf16, optional
    ``bias`` f32 [N], ``relu`` bool, ``act`` bf16 [M, N] (the output is multiplied by (act > 0)).  Column-slice views are fine."""
    recs = []
    for q in jobs:
        segs = q["segs"]
        if not 1 <= len(segs) <= 2:
            raise NativeError("gemm_jobs: one or two K-segments per job")
        y = q["y"]
        yp, ldy = _bf16_rows(y, "y")
        N = y.shape[1]
        xs, ldxs, ws, ldws, ks = [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]
        for i, (x, w) in enumerate(segs):
            xs[i], ldxs[i] = _bf16_rows(x, "x")
            ws[i], ldws[i] = _bf16_rows(w, "w")
            ks[i] = x.shape[1]
            if x.shape[0] != M or y.shape[0] != M or w.shape != (N, ks[i]) or ks[i] % 64 or N % 64:
                raise NativeError(f"gemm_jobs: shapes x {tuple(x.shape)} w {tuple(w.shape)} y {tuple(y.shape)} (M = {M})")
        act = q.get("act")
        ap, lda = (0, 0) if act is None else _bf16_rows(act, "act")
        if act is not None and tuple(act.shape) != (M, N):
            raise NativeError("gemm_jobs: act must be [M, N]")
        bias = q.get("bias")
        recs.append(GemmJob((_vp * 2)(*xs), (_i64 * 2)(*ldxs), (_vp * 2)(*ws), (_i64 * 2)(*ldws), (_i32 * 2)(*ks),
                            None if bias is None else _dev(bias, f32, N, "bias"), ap or None, lda, yp, ldy, N, int(bool(q.get("relu")))))
    if not 1 <= len(recs) <= GEMM_MAX_JOBS:
        raise NativeError(f"gemm_jobs: 1..{GEMM_MAX_JOBS} jobs per launch")
    arr = (GemmJob * len(recs))(*recs)
    _check(load().g2048_gemm_jobs(C.cast(arr, _vp), len(recs), int(M), _stream()), "g2048_gemm_jobs")


def mlp_embed_fwd(boards, wt, bias, y, onehot=None):
    """y[M, 512] (bf16) = relu(bias + sum of the 16 selected rows of wt [496, 512] (bf16, the transposed trunk_in weight)); ``onehot``
    (bf16 [M, 512]) receives the one-hot matrix."""
    M = boards.shape[0]
    bf = torch.bfloat16
    _check(load().g2048_mlp_embed_fwd(_dev(boards, u8, 16 * M, "boards"), _dev(wt, bf, 496 * 512, "wt"), _dev(bias, f32, 512, "bias"),
                                      _dev(y, bf, 512 * M, "y"), _dev(onehot, bf, 512 * M, "onehot", optional=True), M, _stream()),
           "g2048_mlp_embed_fwd")


def mlp_out_fwd(h2, w3, logits, values):
    M = h2.shape[0]
    bf = torch.bfloat16
    _check(load().g2048_mlp_out_fwd(_dev(h2, bf, 1024 * M, "h2"), _dev(w3, bf, 5 * 512, "w3"), _dev(logits, f32, 4 * M, "logits"),
                                    _dev(values, f32, M, "values"), M, _stream()), "g2048_mlp_out_fwd")


def mlp_out_bwd(dlogits, dvalues, h2, w3, dh2):
    """-> partial f32 [rows, 5, 512]: first-stage sums of the output layers' weight gradients."""
    M = h2.shape[0]
    bf = torch.bfloat16
    ws = torch.empty((int(load().g2048_mlp_out_bwd_partial_rows(M)), 5, 512), dtype=f32, device=h2.device)
    _check(load().g2048_mlp_out_bwd(_dev(dlogits, f32, 4 * M, "dlogits"), _dev(dvalues, f32, M, "dvalues"), _dev(h2, bf, 1024 * M, "h2"),
                                    _dev(w3, bf, 5 * 512, "w3"), _dev(dh2, bf, 1024 * M, "dh2"), ws.data_ptr(), M, _stream()),
           "g2048_mlp_out_bwd")
    return ws


def relu_dropout_fwd(x, y, p_drop: float, seed: int, seed_state: int = 0):
    bf = torch.bfloat16
    F = x.shape[-1]
    T = x.numel() // F
    _check(load().g2048_relu_dropout_fwd(_dev(x, bf, T * F, "x"), _dev(y, bf, T * F, "y"), T, F, float(p_drop), int(seed),
                                         seed_state or None, _stream()), "g2048_relu_dropout_fwd")


def relu_dropout_bwd(dy, y, dx, dbias, p_drop: float):
    """dbias None: first stage only -> the workspace, f32 [rows, F] partial sums (for ``reduce_jobs``)."""
    bf = torch.bfloat16
    F = y.shape[-1]
    T = y.numel() // F
    ws = torch.empty(load().g2048_relu_dropout_bwd_workspace_floats(T, F), dtype=f32, device=y.device)
    _check(load().g2048_relu_dropout_bwd(_dev(dy, bf, T * F, "dy"), _dev(y, bf, T * F, "y"), _dev(dx, bf, T * F, "dx"),
                                         _dev(dbias, f32, F, "dbias", optional=True), ws.data_ptr(), T, F, float(p_drop),
                                         _stream()), "g2048_relu_dropout_bwd")
    return ws.view(-1, F) if dbias is None else None


COLSUM_MAX_GROUPS = CONSTANTS["G2048_COLSUM_MAX_GROUPS"]


def colsum(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """f32 column sums of a 2-D bf16/f32 device tensor whose rows are contiguous (any row stride)."""
    if not x.is_cuda or x.dim() != 2 or x.stride(1) != 1 or x.dtype not in (torch.bfloat16, f32):
        raise NativeError(f"colsum: expected a 2-D bf16/f32 device tensor with contiguous rows, got {x.dtype} {tuple(x.shape)} "
                          f"strides {x.stride()}")
    T, N = x.shape
    if out is None:
        out = torch.empty(N, dtype=f32, device=x.device)
    ws = torch.empty(load().g2048_colsum_workspace_floats(T, N), dtype=f32, device=x.device)
    _check(load().g2048_colsum(x.data_ptr(), int(x.dtype == torch.bfloat16), x.stride(0), T, N, ws.data_ptr(),
                               _dev(out, f32, N, "out"), _stream()), "g2048_colsum")
    return out


def colsum_partial(x: torch.Tensor) -> torch.Tensor:
    """First stage of ``colsum`` only -> f32 [rows, N] partial sums (for ``reduce_jobs``); N <= 1024."""
    if not x.is_cuda or x.dim() != 2 or x.stride(1) != 1 or x.dtype not in (torch.bfloat16, f32):
        raise NativeError(f"colsum_partial: expected a 2-D bf16/f32 device tensor with contiguous rows, got {x.dtype} "
                          f"{tuple(x.shape)} strides {x.stride()}")
    T, N = x.shape
    rows = load().g2048_colsum_partial_rows(T, N)
    if rows <= 0:
        raise NativeError(f"colsum_partial: unsupported shape {tuple(x.shape)}")
    ws = torch.empty(load().g2048_colsum_workspace_floats(T, N), dtype=f32, device=x.device)
    _check(load().g2048_colsum(x.data_ptr(), int(x.dtype == torch.bfloat16), x.stride(0), T, N, ws.data_ptr(), None, _stream()),
           "g2048_colsum")
    return ws[:rows * N].view(rows, N)


ReduceJob = STRUCTS["g2048_reduce_job"]


def reduce_jobs(jobs):
    """jobs: list of (src tensor whose first element is part 0 / column 0, dst f32 tensor, part_stride, n, parts[,
    transpose_rows]): dst[c] = sum_p src[p * part_stride + c] (transpose_rows R: the [R][n / R] sum stored as [n / R][R]); all
    of them in one launch (per G2048_REDUCE_MAX_JOBS; the entry point splits longer lists itself)."""
    if not jobs:
        return
    recs = []
    for job in jobs:
        src, dst, stride, n, parts = job[:5]
        tr = int(job[5]) if len(job) > 5 else 0
        if not src.is_cuda or src.dtype not in (torch.bfloat16, f32) or not dst.is_cuda or dst.dtype != f32 \
                or not dst.is_contiguous() or dst.numel() < n:
            raise NativeError(f"reduce_jobs: bad job {src.dtype} {tuple(src.shape)} -> {dst.dtype} {tuple(dst.shape)} (n={n})")
        recs.append(ReduceJob(src.data_ptr(), dst.data_ptr(), int(stride), int(n), int(parts), int(src.dtype == torch.bfloat16), tr))
    arr = (ReduceJob * len(recs))(*recs)
    _check(load().g2048_reduce_jobs(C.cast(arr, _vp), len(recs), _stream()), "g2048_reduce_jobs")


def ppo_loss(logits, values, actions, mask_bits, old_logp, adv, ret, clip_eps: float, c_value: float, c_entropy: float,
             grad_scale=None, running=None):
    """-> (new_logp f32 [M], sums f32 [5], dlogits like logits, dvalues like values); see g2048_ppo_loss.  ``grad_scale``:
    optional device f32 scalar the two gradients are multiplied by; ``running``: optional device f64 [5] the kernel adds the
    five means to."""
    M = actions.numel()
    for name, t in (("logits", logits), ("values", values)):
        if not t.is_cuda or t.dtype not in (torch.bfloat16, f32) or not t.is_contiguous():
            raise NativeError(f"{name}: expected a contiguous bf16/f32 device tensor, got {t.dtype} on {t.device}")
    if logits.numel() != 4 * M or values.numel() != M:
        raise NativeError(f"ppo_loss: logits {tuple(logits.shape)} / values {tuple(values.shape)} do not match M={M}")
    new_logp = torch.empty(M, dtype=f32, device=logits.device)
    sums = torch.empty(5, dtype=f32, device=logits.device)
    dlogits, dvalues = torch.empty_like(logits), torch.empty_like(values)
    _check(load().g2048_ppo_loss(
        logits.data_ptr(), int(logits.dtype == torch.bfloat16), values.data_ptr(), int(values.dtype == torch.bfloat16),
        _dev(actions, u8, M, "actions"), _dev(mask_bits, u8, M, "mask_bits", optional=True), _dev(old_logp, f32, M, "old_logp"),
        _dev(adv, f32, M, "adv"), _dev(ret, f32, M, "ret"), M, float(clip_eps), float(c_value), float(c_entropy),
        new_logp.data_ptr(), sums.data_ptr(), dlogits.data_ptr(), dvalues.data_ptr(),
        _dev(grad_scale, f32, 1, "grad_scale", optional=True), _dev(running, torch.float64, 5, "running", optional=True),
        _stream()), "g2048_ppo_loss")
    return new_logp, sums, dlogits, dvalues


def distill_loss_workspace_floats(M: int) -> int:
    """The f32 elements of workspace ``distill_loss`` needs for M samples; raises outside 1 .. G2048_PPO_LOSS_MAX_BATCH."""
    n = int(load().g2048_distill_loss_workspace_floats(int(M)))
    if n < 0:
        raise NativeError(f"distill_loss: M={M} is outside 1 .. {CONSTANTS['G2048_PPO_LOSS_MAX_BATCH']}")
    return n


def distill_loss(logits, values, mask_bits, teacher_q, value_target, tau: float, c_value: float, c_entropy: float, grad_scale=None,
                 running=None, workspace=None, out=None):
    """-> (new_logp f32 [M], sums f32 [5], dlogits like logits, dvalues like values or None); see g2048_distill_loss.  ``values``
    and ``value_target`` are None together (no critic term).  ``grad_scale`` / ``running`` as in ``ppo_loss``; ``workspace``: f32
    of ``distill_loss_workspace_floats(M)`` elements (allocated if None); ``out``: pre-allocated (new_logp, sums, dlogits, dvalues)."""
    if not isinstance(teacher_q, torch.Tensor) or not teacher_q.is_cuda:
        raise NativeError(f"teacher_q: expected a HIP device tensor, got {getattr(teacher_q, 'device', None)} (no CPU path exists)")
    M = teacher_q.numel() // 4
    if (values is None) != (value_target is None):
        raise NativeError("distill_loss: values and value_target are given together or not at all")
    for name, t in (("logits", logits), ("values", values)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype not in (torch.bfloat16, f32) or not t.is_contiguous():
            raise NativeError(f"{name}: expected a contiguous bf16/f32 device tensor, got {t.dtype} on {t.device}")
    if logits.numel() != 4 * M or (values is not None and values.numel() != M):
        raise NativeError(f"distill_loss: logits {tuple(logits.shape)} / values "
                          f"{None if values is None else tuple(values.shape)} do not match M={M}")
    n_ws = distill_loss_workspace_floats(M)
    if workspace is None:
        workspace = torch.empty(n_ws, dtype=f32, device=logits.device)
    if out is None:
        out = (torch.empty(M, dtype=f32, device=logits.device), torch.empty(5, dtype=f32, device=logits.device),
               torch.empty_like(logits), None if values is None else torch.empty_like(values))
    new_logp, sums, dlogits, dvalues = out
    if dlogits.dtype != logits.dtype or not dlogits.is_cuda or dlogits.numel() < 4 * M or not dlogits.is_contiguous():
        raise NativeError("dlogits: expected a contiguous device tensor like logits")
    if (dvalues is None) != (values is None) or (dvalues is not None and (
            dvalues.dtype != values.dtype or not dvalues.is_cuda or dvalues.numel() < M or not dvalues.is_contiguous())):
        raise NativeError("dvalues: expected a contiguous device tensor like values (None with it)")
    _check(load().g2048_distill_loss(
        logits.data_ptr(), int(logits.dtype == torch.bfloat16), None if values is None else values.data_ptr(),
        int(values is not None and values.dtype == torch.bfloat16), _dev(mask_bits, u8, M, "mask_bits", optional=True),
        _dev(teacher_q, f32, 4 * M, "teacher_q"), _dev(value_target, f32, M, "value_target", optional=True), M, float(tau),
        float(c_value), float(c_entropy), _dev(new_logp, f32, M, "new_logp"), _dev(sums, f32, 5, "sums"), dlogits.data_ptr(),
        None if dvalues is None else dvalues.data_ptr(), _dev(grad_scale, f32, 1, "grad_scale", optional=True),
        _dev(running, torch.float64, 5, "running", optional=True), _dev(workspace, f32, n_ws, "workspace"), _stream()),
        "g2048_distill_loss")
    return new_logp, sums, dlogits, dvalues


def distill_gather(idx, boards, masks, teacher_q, value_target=None, out=None):
    """-> dict(obs u8 [M,16], masks u8 [M], q f32 [M,4], vt f32 [M] or None) = rows idx (clamped) of the imitation ring; ``out``:
    pre-allocated tensors of that layout.  See g2048_distill_gather."""
    M, N = idx.numel(), masks.numel()
    dev = boards.device
    if out is None:
        out = dict(obs=torch.empty((M, 16), dtype=u8, device=dev), masks=torch.empty(M, dtype=u8, device=dev),
                   q=torch.empty((M, 4), dtype=f32, device=dev),
                   vt=None if value_target is None else torch.empty(M, dtype=f32, device=dev))
    _check(load().g2048_distill_gather(
        _dev(idx, i64, M, "idx"), M, N, _dev(boards, u8, 16 * N, "boards"), _dev(masks, u8, N, "masks"),
        _dev(teacher_q, f32, 4 * N, "teacher_q"), _dev(value_target, f32, N, "value_target", optional=True),
        _dev(out["obs"], u8, 16 * M, "o_boards"), _dev(out["masks"], u8, M, "o_masks"), _dev(out["q"], f32, 4 * M, "o_q"),
        _dev(out.get("vt"), f32, M, "o_vt", optional=True), _stream()), "g2048_distill_gather")
    return out


def linear_ok(x2: torch.Tensor, weight: torch.Tensor) -> bool:
    """Shapes/strides g2048_linear_bf16 takes: x2 [T, K] and weight [N, K] bf16 on the device with contiguous rows."""
    return (x2.is_cuda and x2.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and x2.dim() == 2
            and weight.dim() == 2 and x2.stride(1) == 1 and weight.stride(1) == 1 and x2.shape[1] == weight.shape[1]
            and x2.shape[1] % 128 == 0 and weight.shape[0] % 128 == 0 and x2.stride(0) % 8 == 0 and weight.stride(0) % 8 == 0
            and x2.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0 and x2.shape[0] > 0)


def _out_rows(out: torch.Tensor, T: int, N: int, name: str) -> int:
    """The leading dimension of a caller's bf16 [T, N] output: contiguous, or a row view (unit inner stride) of a wider buffer."""
    if not out.is_cuda or out.dtype != torch.bfloat16 or out.dim() != 2 or tuple(out.shape) != (T, N) or out.stride(1) != 1:
        raise NativeError(f"{name}: out must be a bf16 [{T}, {N}] device tensor with contiguous rows")
    return N if out.is_contiguous() else out.stride(0)


def linear_bf16(x2: torch.Tensor, weight: torch.Tensor, bias_f32=None, out=None) -> torch.Tensor:
    """out[T, N] (bf16) = x2[T, K] @ weight[N, K]^T (+ bias f32 [N]).  ``out``: contiguous with at least T * N elements, or a [T, N] row
    view of a wider buffer (its row stride becomes ldy)."""
    if not linear_ok(x2, weight):
        raise NativeError(f"linear_bf16: unsupported operands {tuple(x2.shape)} {x2.dtype} x {tuple(weight.shape)} {weight.dtype}")
    T, K = x2.shape
    N = weight.shape[0]
    if out is None:
        out = torch.empty((T, N), dtype=torch.bfloat16, device=x2.device)
    if out.is_contiguous():
        out_ptr, ldy = _dev(out, torch.bfloat16, T * N, "out"), N
    else:
        out_ptr, ldy = out.data_ptr(), _out_rows(out, T, N, "linear_bf16")
    _check(load().g2048_linear_bf16(x2.data_ptr(), x2.stride(0), weight.data_ptr(), weight.stride(0),
                                    _dev(bias_f32, f32, N, "bias", optional=True), out_ptr, ldy, T, K, N, _stream()), "g2048_linear_bf16")
    return out


def linear_relu_dropout(x2: torch.Tensor, weight: torch.Tensor, bias_f32: torch.Tensor, p_drop: float, seed: int = 0,
                        seed_state: int = 0, want_mask: bool = False, out=None, mask=None):
    """dropout(relu(x2 @ weight^T + bias)) -> bf16 [T, N] in one launch (K <= 256); see g2048_linear_relu_dropout_bf16.
    ``want_mask``: -> (y, mask) with the opaque bit mask ``linear_mask_bwd`` reads.  ``out`` (bf16 [T, N], contiguous or a row view of a
    wider buffer) and ``mask`` (uint8, ``g2048_ffn_mask_bytes`` elements, 8-byte aligned; implies ``want_mask``) are written in place of
    fresh allocations."""
    if not linear_ok(x2, weight) or x2.shape[1] > 256:
        raise NativeError(f"linear_relu_dropout: unsupported operands {tuple(x2.shape)} {x2.dtype} x {tuple(weight.shape)}")
    T, K = x2.shape
    N = weight.shape[0]
    if out is None:
        out = torch.empty((T, N), dtype=torch.bfloat16, device=x2.device)
    ldy = _out_rows(out, T, N, "linear_relu_dropout")
    want_mask = want_mask or mask is not None
    if mask is None:
        mask = torch.empty(load().g2048_ffn_mask_bytes(T, N), dtype=u8, device=x2.device) if want_mask else None
    elif (mask.dtype != u8 or not mask.is_cuda or not mask.is_contiguous() or mask.numel() != load().g2048_ffn_mask_bytes(T, N)
          or mask.data_ptr() % 8):
        raise NativeError(f"linear_relu_dropout: the mask buffer does not fit a [{T}, {N}] call")
    _check(load().g2048_linear_relu_dropout_bf16(x2.data_ptr(), x2.stride(0), weight.data_ptr(), weight.stride(0),
                                                 _dev(bias_f32, f32, N, "bias"), out.data_ptr(), ldy, T, K, N, float(p_drop),
                                                 int(seed) & (2 ** 64 - 1), seed_state or None,
                                                 mask.data_ptr() if want_mask else None, _stream()),
           "g2048_linear_relu_dropout_bf16")
    return (out, mask) if want_mask else out


def linear_mask_bwd(dy2: torch.Tensor, weight_t: torch.Tensor, mask: torch.Tensor, p_drop: float, final: bool = True, out=None, db=None,
                    workspace=None):
    """-> (dz bf16 [T, N], dbias f32 [N]): dz = (dy2 @ weight_t^T) / (1 - p) where the forward's output was non-zero
    (``mask`` from ``linear_relu_dropout(..., want_mask=True)`` with the same T and N); see g2048_linear_mask_bwd_bf16.
    ``final`` False: (dz, partial sums f32 [rows, N]) for ``reduce_jobs``.  ``out`` (bf16 [T, N], contiguous or a row view of a wider
    buffer), ``db`` (f32 [N]) and ``workspace`` (f32, ``g2048_linear_mask_bwd_workspace_floats`` elements) are written in place of fresh
    allocations."""
    if not linear_ok(dy2, weight_t) or dy2.shape[1] > 256:
        raise NativeError(f"linear_mask_bwd: unsupported operands {tuple(dy2.shape)} {dy2.dtype} x {tuple(weight_t.shape)}")
    T, K = dy2.shape
    N = weight_t.shape[0]
    if mask.dtype != u8 or not mask.is_cuda or mask.numel() != load().g2048_ffn_mask_bytes(T, N) or mask.data_ptr() % 8:
        raise NativeError(f"linear_mask_bwd: the mask does not belong to a [{T}, {N}] forward call")
    dz = torch.empty((T, N), dtype=torch.bfloat16, device=dy2.device) if out is None else out
    lddz = _out_rows(dz, T, N, "linear_mask_bwd")
    if final and db is None:
        db = torch.empty(N, dtype=f32, device=dy2.device)
    ws_floats = load().g2048_linear_mask_bwd_workspace_floats(T, N)
    ws = torch.empty(ws_floats, dtype=f32, device=dy2.device) if workspace is None else workspace
    _check(load().g2048_linear_mask_bwd_bf16(dy2.data_ptr(), dy2.stride(0), weight_t.data_ptr(), weight_t.stride(0),
                                             mask.data_ptr(), dz.data_ptr(), lddz, _dev(db, f32, N, "db") if final else None,
                                             _dev(ws, f32, ws_floats, "workspace"), T, K, N, float(p_drop), _stream()),
           "g2048_linear_mask_bwd_bf16")
    if final:
        return dz, db
    rows = load().g2048_linear_mask_bwd_partial_rows(T, N)
    return dz, ws.view(-1)[:rows * N].view(rows, N)


def embed_fwd(boards, wt, pe, cls, x0, p_drop: float = 0.0, seed: int = 0, seed_state: int = 0, ln=None):
    """wt: the class-major table f32 [31, 256], or the nn.Linear weight f32 [256, 31] itself (read in place).  ``ln`` = (gamma f32
    [256], beta f32 [256], eps, h bf16 [M, 17, 256], mean f32 [M * 17], rstd f32 [M * 17]): also the LayerNorm of every row
    (``g2048_embed_ln_fwd``)."""
    M = boards.numel() // 16
    w_ld = 0 if tuple(wt.shape) == (31, 256) else int(wt.shape[1])
    if w_ld and (wt.dim() != 2 or wt.shape[0] != 256 or w_ld < 31):
        raise NativeError(f"embed_fwd: weight must be [31, 256] or [256, >= 31], got {tuple(wt.shape)}")
    if ln is not None:
        gamma, beta, eps, h, mean, rstd = ln
        _check(load().g2048_embed_ln_fwd(_dev(boards, u8, 16 * M, "boards"), _dev(wt, f32, 31 * 256, "wt"), w_ld,
                                         _dev(pe, f32, 16 * 256, "pe"), _dev(cls, f32, 256, "cls"), _dev(x0, f32, M * 17 * 256, "x0"), M,
                                         float(p_drop), int(seed), seed_state or None, _dev(gamma, f32, 256, "gamma"),
                                         _dev(beta, f32, 256, "beta"), float(eps), _dev(h, torch.bfloat16, M * 17 * 256, "h"),
                                         _dev(mean, f32, M * 17, "mean"), _dev(rstd, f32, M * 17, "rstd"), _stream()), "g2048_embed_ln_fwd")
        return
    _check(load().g2048_embed_fwd(_dev(boards, u8, 16 * M, "boards"), _dev(wt, f32, 31 * 256, "wt"), w_ld,
                                  _dev(pe, f32, 16 * 256, "pe"),
                                  _dev(cls, f32, 256, "cls"), _dev(x0, f32, M * 17 * 256, "x0"), M, float(p_drop), int(seed),
                                  seed_state or None, _stream()), "g2048_embed_fwd")


def embed_bwd(boards, dx0, dwt_dcls, p_drop: float = 0.0, seed: int = 0, seed_state: int = 0):
    """dwt_dcls None: first stage only -> the workspace, f32 [rows, 32 * 256] partial sums (for ``reduce_jobs``)."""
    M = boards.numel() // 16
    ws = torch.empty(load().g2048_embed_bwd_workspace_floats(M), dtype=f32, device=dx0.device)
    _check(load().g2048_embed_bwd(_dev(boards, u8, 16 * M, "boards"), _dev(dx0, f32, M * 17 * 256, "dx0"),
                                  _dev(dwt_dcls, f32, 32 * 256, "dwt_dcls", optional=True), ws.data_ptr(), M, float(p_drop),
                                  int(seed), seed_state or None, _stream()), "g2048_embed_bwd")
    return ws.view(-1, 32 * 256) if dwt_dcls is None else None


OPT_CHUNK, OPT_MAX_GROUPS = CONSTANTS["G2048_OPT_CHUNK"], CONSTANTS["G2048_OPT_MAX_GROUPS"]
OptChunk, OptGroup, LambGroup = STRUCTS["g2048_opt_chunk"], STRUCTS["g2048_opt_group"], STRUCTS["g2048_lamb_group"]
OPT_CHUNK_BYTES = C.sizeof(OptChunk)


def opt_chunk_table(params, offsets, groups, device, shadows=None) -> torch.Tensor:
    """The device-resident chunk table of g2048_opt_step (u8 tensor holding g2048_opt_chunk records): parameter i (a
    contiguous f32 device tensor) has its gradient/moments at element offsets[i] of the flat buffers and belongs to
    hyper-parameter group groups[i].  ``shadows``: optional {id(parameter): (bf16 copy, bf16 transposed copy or None[, bf16
    fragment-packed copy or None, bf16 fragment-packed transposed copy or None])} the step keeps up to date."""
    recs = []
    shadows = shadows or {}
    for p, off, grp in zip(params, offsets, groups):
        if not p.is_cuda or p.dtype != f32 or not p.is_contiguous() or p.data_ptr() % 16 or off % 4:
            raise NativeError(f"opt_chunk_table: parameter {tuple(p.shape)} {p.dtype} on {p.device} (offset {off}) is not a "
                              "contiguous 16-byte aligned f32 device tensor at a flat offset that is a multiple of 4")
        n = p.numel()
        sh, sh_t, sh_p, sh_tp = (tuple(shadows.get(id(p), ())) + (None,) * 4)[:4]
        for t in (sh, sh_t, sh_p, sh_tp):
            if t is not None and (t.dtype != torch.bfloat16 or not t.is_cuda or not t.is_contiguous() or t.numel() != n):
                raise NativeError(f"opt_chunk_table: shadow of a {tuple(p.shape)} parameter must be a contiguous bf16 tensor of {n} elements")
        if sh_t is not None and (p.dim() != 2 or tuple(sh_t.shape) != tuple(p.shape[::-1])):
            raise NativeError("opt_chunk_table: a transposed shadow needs a 2-D parameter and the transposed shape")
        if sh_p is not None and (p.dim() != 2 or p.shape[0] % 32 or p.shape[1] % 16 or sh_p.data_ptr() % 16):
            raise NativeError("opt_chunk_table: a packed shadow needs a 2-D parameter with rows % 32 == 0 and cols % 16 == 0")
        if sh_tp is not None and (p.dim() != 2 or p.shape[1] % 32 or p.shape[0] % 16 or sh_tp.data_ptr() % 16):
            raise NativeError("opt_chunk_table: a packed transposed shadow needs a 2-D parameter with cols % 32 == 0 and rows % 16 == 0")
        rows, cols = (p.shape[0], p.shape[1]) if p.dim() == 2 else (1, max(n, 1))
        for c0 in range(0, n, OPT_CHUNK):
            recs.append(OptChunk(p.data_ptr() + 4 * c0, off + c0, min(OPT_CHUNK, n - c0), grp, sh.data_ptr() if sh is not None else None,
                                 sh_t.data_ptr() if sh_t is not None else None, sh_p.data_ptr() if sh_p is not None else None,
                                 sh_tp.data_ptr() if sh_tp is not None else None, c0, rows, cols, 0))
    arr = (OptChunk * len(recs))(*recs)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=u8)
    return host.to(device)


def opt_workspace(n_chunks: int, device) -> torch.Tensor:
    """Zeroed workspace for g2048_opt_step (one partial sum per chunk, then the per-group constants)."""
    return torch.zeros(load().g2048_opt_workspace_floats(n_chunks), dtype=f32, device=device)


def opt_step(table, n_chunks: int, grads, exp_avg, exp_avg_sq, groups, max_grad_norm: float, steps, scale, growth_tracker,
             growth: float, backoff: float, growth_interval: int, workspace, info=None):
    """Clip + AdamW (+ GradScaler unscale / skip / update when ``scale`` is given) for every chunk of ``table``; ``groups``:
    list of (lr, beta1, beta2, eps, weight_decay)."""
    if len(groups) > OPT_MAX_GROUPS:
        raise NativeError(f"opt_step: {len(groups)} parameter groups, at most {OPT_MAX_GROUPS} are supported")
    g = (OptGroup * len(groups))(*[OptGroup(*map(float, t)) for t in groups])
    n = grads.numel()
    _check(load().g2048_opt_step(
        table.data_ptr(), n_chunks, _dev(grads, f32, None, "grads"), _dev(exp_avg, f32, n, "exp_avg"),
        _dev(exp_avg_sq, f32, n, "exp_avg_sq"), C.cast(g, _vp), len(groups), float(max_grad_norm if max_grad_norm else 0.0),
        _dev(steps, f32, 1, "steps"), steps.numel(), _dev(scale, f32, 1, "scale", optional=True),
        _dev(growth_tracker, torch.int32, 1, "growth_tracker", optional=True), float(growth), float(backoff),
        int(growth_interval), _dev(workspace, f32, None, "workspace"), _dev(info, f32, 2, "info", optional=True), _stream()),
        "g2048_opt_step")


def lamb_workspace(n_chunks: int, device) -> torch.Tensor:
    """Zeroed workspace for g2048_lamb_step (three partial sums per chunk, the step's flags, the per-group constants)."""
    return torch.zeros(load().g2048_lamb_workspace_floats(n_chunks), dtype=f32, device=device)


def lamb_step(table, n_chunks: int, grads, exp_avg, exp_avg_sq, groups, max_grad_norm: float, lamb_max_grad_norm, steps, scale,
              growth_tracker, growth: float, backoff: float, growth_interval: int, workspace, info=None):
    """Clip + LAMB (+ GradScaler unscale / skip / update when ``scale`` is given) for every chunk of ``table`` (an
    ``opt_chunk_table``); ``groups``: list of (lr, beta1, beta2, beta3, eps, weight_decay, bias_correction, adapt, trust_clip);
    ``lamb_max_grad_norm``: Lamb's own clip threshold, None or 0 for none."""
    if len(groups) > OPT_MAX_GROUPS:
        raise NativeError(f"lamb_step: {len(groups)} parameter groups, at most {OPT_MAX_GROUPS} are supported")
    g = (LambGroup * len(groups))(*[LambGroup(*map(float, t[:6]), *(int(bool(x)) for x in t[6:9]), 0) for t in groups])
    n = grads.numel()
    _check(load().g2048_lamb_step(
        table.data_ptr(), n_chunks, _dev(grads, f32, None, "grads"), _dev(exp_avg, f32, n, "exp_avg"),
        _dev(exp_avg_sq, f32, n, "exp_avg_sq"), C.cast(g, _vp), len(groups), float(max_grad_norm if max_grad_norm else 0.0),
        float(lamb_max_grad_norm if lamb_max_grad_norm else 0.0), _dev(steps, f32, 1, "steps"), steps.numel(),
        _dev(scale, f32, 1, "scale", optional=True), _dev(growth_tracker, torch.int32, 1, "growth_tracker", optional=True),
        float(growth), float(backoff), int(growth_interval), _dev(workspace, f32, None, "workspace"),
        _dev(info, f32, 2, "info", optional=True), _stream()), "g2048_lamb_step")


def gather_minibatch(idx, boards, actions, masks, logp, adv, ret, out=None):
    """-> dict(obs u8 [M,16], actions u8 [M], masks u8 [M], old_lp, adv, ret f32 [M]) = rows idx of the buffer (``out``:
    pre-allocated tensors of that layout, e.g. the static inputs of a captured graph)."""
    M, N = idx.numel(), actions.numel()
    dev = boards.device
    if out is None:
        out = dict(obs=torch.empty((M, 16), dtype=u8, device=dev), actions=torch.empty(M, dtype=u8, device=dev),
                   masks=torch.empty(M, dtype=u8, device=dev), old_lp=torch.empty(M, dtype=f32, device=dev),
                   adv=torch.empty(M, dtype=f32, device=dev), ret=torch.empty(M, dtype=f32, device=dev))
    _check(load().g2048_gather_minibatch(
        _dev(idx, i64, M, "idx"), M, N, _dev(boards, u8, 16 * N, "boards"), _dev(actions, u8, N, "actions"),
        _dev(masks, u8, N, "masks"), _dev(logp, f32, N, "logp"), _dev(adv, f32, N, "adv"), _dev(ret, f32, N, "ret"),
        _dev(out["obs"], u8, 16 * M, "o_boards"), _dev(out["actions"], u8, M, "o_actions"), _dev(out["masks"], u8, M, "o_masks"),
        _dev(out["old_lp"], f32, M, "o_logp"), _dev(out["adv"], f32, M, "o_adv"), _dev(out["ret"], f32, M, "o_ret"), _stream()),
        "g2048_gather_minibatch")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the 2048-row tail of the update (csrc/g2048_tail.hip)
# ---------------------------------------------------------------------------------------------------------------------
TAIL_MASK_TILES, DW_MAX_JOBS = CONSTANTS["G2048_TAIL_MASK_TILES"], CONSTANTS["G2048_DW_MAX_JOBS"]
TailWeights, TailWeightsT = STRUCTS["g2048_tail_weights"], STRUCTS["g2048_tail_weights_t"]
TailSaved, TailGrads, DwJob = STRUCTS["g2048_tail_saved"], STRUCTS["g2048_tail_grads"], STRUCTS["g2048_dw_job"]


def pack_fragments(x: torch.Tensor) -> torch.Tensor:
    """Row-major [rows, cols] (rows % 32 == 0, cols % 16 == 0) -> the fragment-packed layout of include/g2048.h, as a flat tensor."""
    R, Cc = x.shape
    return x.reshape(R // 32, 32, Cc // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1).contiguous()


def unpack_fragments(flat: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """Inverse of ``pack_fragments``: flat packed tensor -> row-major [rows, cols]."""
    return flat.reshape(rows // 32, cols // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(rows, cols)


_TAIL_SAVED_ROWS = dict(oT=256, h2T=256, uT=1024, featsT=256, a1T=512, a2T=512, c1T=512, c2T=512)
_TAIL_GRAD_ROWS = dict(daoT=256, dzT=1024, df2T=256, da1T=512, da2T=512, dlT=32, dc1T=512, dc2T=512, dvT=32)


class TailBuffers:
    """Device buffers of one g2048_cls_tail_fwd / _bwd pair for M rows (allocated once per minibatch size and reused: every
    element that is read is rewritten by each forward / backward; dlT / dvT rows that are never written stay zero)."""

    def unpacked(self, name: str) -> torch.Tensor:
        """Row-major [rows, ld] view-copy of a packed transposed buffer (tests / debugging)."""
        t = self.saved[name] if name in self.saved else self.grads[name]
        return unpack_fragments(t, self.rows[name], self.ld)

    def __init__(self, M: int, device):
        bf = torch.bfloat16
        self.M, self.blocks = int(M), (int(M) + 31) // 32
        self.ld = 32 * self.blocks
        # slices of the row axis in g2048_dweight_t: 8 (one per XCD) when every slice is a whole number of 16-row k-steps
        self.slices = next(s for s in (8, 4, 2, 1) if self.ld % (16 * s) == 0)
        z = lambda *shape, dtype=bf: torch.zeros(shape, dtype=dtype, device=device)
        self.saved = dict(x_mid=z(self.M, 256, dtype=f32), mean=z(self.M, dtype=f32), rstd=z(self.M, dtype=f32),
                          masks=z(self.blocks, TAIL_MASK_TILES, 64, dtype=torch.int16))
        # transposed activations / gradients, fragment-packed (``unpack_fragments(t, rows, ld)`` gives [rows, ld]): flat tensors
        self.saved.update({k: z(rows * self.ld) for k, rows in _TAIL_SAVED_ROWS.items()})
        self.grads = {k: z(rows * self.ld) for k, rows in _TAIL_GRAD_ROWS.items()}
        self.rows = dict(_TAIL_SAVED_ROWS, **_TAIL_GRAD_ROWS)
        self.grads["ln_partial"] = z(self.blocks, 512, dtype=f32)
        self.saved_c = TailSaved(*[self.saved[n].data_ptr() for n, _ in TailSaved._fields_[:-1]], self.ld)
        self.grads_c = TailGrads(*[self.grads[n].data_ptr() for n, _ in TailGrads._fields_])
        self.logits, self.values = z(self.M, 4, dtype=f32), z(self.M, dtype=f32)
        self.d_o, self.dx_cls = z(self.M, 256), z(self.M, 256, dtype=f32)
        # weight-gradient partials [slices][N][K] / [slices][N] per Linear: (dyT key, xT key, N (padded to 32), K, has bias)
        self.dw_spec = dict(wo=("daoT", "oT", 256, 256, True), w1=("dzT", "h2T", 1024, 256, True), w2=("df2T", "uT", 256, 1024, True),
                            a1=("da1T", "featsT", 512, 256, True), a2=("da2T", "a1T", 512, 512, True), a3=("dlT", "a2T", 32, 512, False),
                            c1=("dc1T", "featsT", 512, 256, True), c2=("dc2T", "c1T", 512, 512, True), c3=("dvT", "c2T", 32, 512, False))
        self.dw = {k: z(self.slices, n, kk, dtype=f32) for k, (_, _, n, kk, _) in self.dw_spec.items()}
        self.db = {k: z(self.slices, n, dtype=f32) for k, (_, _, n, _, b) in self.dw_spec.items() if b}


def _ptr_struct(cls, tensors: dict, dtypes: dict):
    vals = []
    for name, _ in cls._fields_:
        t = tensors[name]
        want = dtypes.get(name, torch.bfloat16)
        if not t.is_cuda or t.dtype != want or not t.is_contiguous() or t.data_ptr() % 16:
            raise NativeError(f"{cls.__name__}.{name}: expected a contiguous, 16-byte aligned {want} device tensor, got {t.dtype} "
                              f"on {t.device}")
        vals.append(t.data_ptr())
    return cls(*vals)


_TAIL_F32 = {n: f32 for n in ("bo", "b1", "b2", "ab1", "ab2", "cb1", "cb2", "ln_g", "ln_b")}


def tail_weights(tensors: dict) -> TailWeights:
    """bf16 weights (nn.Linear layout) + f32 biases / norm2 parameters by field name -> the C struct (the caller keeps them alive)."""
    return _ptr_struct(TailWeights, tensors, _TAIL_F32)


def tail_weights_t(tensors: dict) -> TailWeightsT:
    return _ptr_struct(TailWeightsT, tensors, _TAIL_F32)


def cls_tail_fwd(o, x_cls_ptr: int, x_row_stride: int, W: TailWeights, buf: TailBuffers, eps: float, p_drop: float, seed: int,
                 seed_state: int = 0):
    """o bf16 [M, 256]; x_cls_ptr: raw device address of f32 rows (element stride x_row_stride) the caller keeps alive.
    -> (buf.logits f32 [M, 4], buf.values f32 [M])."""
    _check(load().g2048_cls_tail_fwd(_dev(o, torch.bfloat16, 256 * buf.M, "o"), x_cls_ptr, int(x_row_stride), C.byref(W),
                                     C.byref(buf.saved_c), buf.logits.data_ptr(), buf.values.data_ptr(), buf.M, float(eps),
                                     float(p_drop), int(seed), seed_state or None, _stream()), "g2048_cls_tail_fwd")
    return buf.logits, buf.values


def cls_tail_bwd(dlogits, dvalues, WT: TailWeightsT, buf: TailBuffers, p_drop: float, seed: int, seed_state: int = 0):
    """-> (buf.d_o bf16 [M, 256], buf.dx_cls f32 [M, 256]); dY^T of every Linear and the LayerNorm partials land in buf.grads."""
    _check(load().g2048_cls_tail_bwd(_dev(dlogits, f32, 4 * buf.M, "dlogits"), _dev(dvalues, f32, buf.M, "dvalues"), C.byref(WT),
                                     C.byref(buf.saved_c), C.byref(buf.grads_c), buf.d_o.data_ptr(), buf.dx_cls.data_ptr(), buf.M,
                                     float(p_drop), int(seed), seed_state or None, _stream()), "g2048_cls_tail_bwd")
    return buf.d_o, buf.dx_cls


def dweight_ok(dy2: torch.Tensor, x2: torch.Tensor, slices: int) -> bool:
    """Operands ``g2048_dweight_bf16`` takes: bf16 [T, N] / [T, K] row views (unit inner stride), N and K multiples of 128,
    T a multiple of 64 * slices."""
    if dy2.dim() != 2 or x2.dim() != 2 or dy2.shape[0] != x2.shape[0]:
        return False
    T, N, K = dy2.shape[0], dy2.shape[1], x2.shape[1]
    for t in (dy2, x2):
        if not t.is_cuda or t.dtype != torch.bfloat16 or t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16 or t.stride(0) >= 1 << 27:
            return False
    return N % 128 == 0 and K % 128 == 0 and T > 0 and T % (64 * slices) == 0 and (slices < 8 or slices % 8 == 0)


def dweight_parts(dy2: torch.Tensor, x2: torch.Tensor, slices: int, out: torch.Tensor = None, block_rows: int = 0, colsum: bool = False,
                  colsum_out: torch.Tensor = None):
    """bf16 [slices, N, K] whose sum over the first axis is dY^T X (``g2048_dweight_bf16``); with ``colsum`` also f32 [slices, N] whose
    sum over the first axis is ``dy2.sum(0)``: -> (parts, column sums).  ``colsum_out`` (f32, slices * N elements; implies ``colsum``) is
    written in place of a fresh allocation."""
    if not dweight_ok(dy2, x2, slices):
        raise NativeError(f"dweight_parts: operands {tuple(dy2.shape)} x {tuple(x2.shape)} with {slices} slices are not supported")
    T, N, K = dy2.shape[0], dy2.shape[1], x2.shape[1]
    if out is None:
        out = torch.empty((slices, N, K), dtype=torch.bfloat16, device=dy2.device)
    colsum = colsum or colsum_out is not None
    cs = None
    if colsum:
        cs = torch.empty((slices, N), dtype=f32, device=dy2.device) if colsum_out is None else colsum_out
    _check(load().g2048_dweight_bf16(dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0), _dev(out, torch.bfloat16, slices * N * K, "parts"),
                                     None if cs is None else _dev(cs, f32, slices * N, "colsum"), T, N, K, int(slices), int(block_rows), _stream()),
           "g2048_dweight_bf16")
    return (out, cs) if colsum else out


DwgJob = STRUCTS["g2048_dwg_job"]
DWG_MAX_JOBS = CONSTANTS["G2048_DWG_MAX_JOBS"]


def dweight_jobs_plan(shapes, big_cells: int = -1, cus: int = 0):
    """The block shapes ``g2048_dweight_jobs_tiled`` gives a launch of jobs of these (N, K, slices) on ``cus`` compute units: per job the
    number of leading [256 x 256] cells computed as one block each (the rest: [128 x 128] blocks).  Host arithmetic only."""
    recs = [DwgJob(None, None, None, None, 0, 0, 0, N, K, slices, 0) for N, K, slices in shapes]
    arr, out = (DwgJob * len(recs))(*recs), (_i32 * len(recs))()
    _check(load().g2048_dweight_jobs_plan(C.cast(arr, _vp), len(recs), int(big_cells), int(cus), C.cast(out, _vp)), "g2048_dweight_jobs_plan")
    return list(out)


def dweight_jobs(jobs, big_cells: int = -1):
    """Several ``dweight_parts`` products in one launch per ``DWG_MAX_JOBS`` (``g2048_dweight_jobs_tiled``).  jobs: (dy2, x2, parts bf16
    (or f32: the job's ``parts_f32`` flag) [slices, N, K], colsum f32 [slices, N] or None); slices (= parts.shape[0]) a multiple of 8.
    ``big_cells``: how many [256 x 256] cells of each launch's jobs, in job order, are computed as one block (the rest as [128 x 128]
    blocks; the partials are the same bits either way); -1: the entry point's choice for the device."""
    recs = []
    for dy2, x2, parts, cs in jobs:
        slices = parts.shape[0]
        if not dweight_ok(dy2, x2, slices) or slices % 8:
            raise NativeError(f"dweight_jobs: operands {tuple(dy2.shape)} x {tuple(x2.shape)} with {slices} slices are not supported")
        T, N, K = dy2.shape[0], dy2.shape[1], x2.shape[1]
        if parts.dtype not in (torch.bfloat16, f32):
            raise NativeError(f"dweight_jobs: parts must be bf16 or f32, got {parts.dtype}")
        recs.append(DwgJob(dy2.data_ptr(), x2.data_ptr(), _dev(parts, parts.dtype, slices * N * K, "parts"),
                           None if cs is None else _dev(cs, f32, slices * N, "colsum"), dy2.stride(0), x2.stride(0), T, N, K, slices,
                           int(parts.dtype == f32)))
    for i in range(0, len(recs), DWG_MAX_JOBS):
        chunk = recs[i:i + DWG_MAX_JOBS]
        arr = (DwgJob * len(chunk))(*chunk)
        _check(load().g2048_dweight_jobs_tiled(C.cast(arr, _vp), len(chunk), int(big_cells), _stream()), "g2048_dweight_jobs_tiled")


def dweight_t(jobs, ld: int, m: int, slices: int):
    """jobs: list of (dyT, xT, dw f32 [slices, N, K], db f32 [slices, N] or None); dyT / xT: fragment-packed bf16 of N * ld / K * ld
    elements (``pack_fragments`` of the [N, ld] / [K, ld] matrices)."""
    recs = []
    for dyT, xT, dw, db in jobs:
        N, K = dw.shape[1], dw.shape[2]
        for t, dt, name in ((dyT, torch.bfloat16, "dyT"), (xT, torch.bfloat16, "xT"), (dw, f32, "dw")):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise NativeError(f"dweight_t: {name} must be a contiguous {dt} device tensor")
        if dyT.numel() != N * ld or xT.numel() != K * ld or dw.shape[0] != slices or (db is not None and db.numel() != slices * N):
            raise NativeError(f"dweight_t: {dyT.numel()} x {xT.numel()} elements -> {tuple(dw.shape)} do not fit ld={ld}")
        recs.append(DwJob(dyT.data_ptr(), xT.data_ptr(), dw.data_ptr(), None if db is None else _dev(db, f32, slices * N, "db"), N, K))
    arr = (DwJob * len(recs))(*recs)
    _check(load().g2048_dweight_t(C.cast(arr, _vp), len(recs), int(ld), int(m), int(slices), _stream()), "g2048_dweight_t")

