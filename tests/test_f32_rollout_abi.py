"""The split-fp16 fp32-rollout entry points on a machine without a GPU: exported, bound, argument checks, and the switch.  CPU only."""
import ctypes as C

import numpy as np
import torch

from src.g2048 import native as nv

NEW = ("g2048_f32split_pack", "g2048_f32split_gemm", "g2048_attn_fwd_f32", "g2048_embed_ln_f32")


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(nv.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n) and n in nv.SIGNATURES
    assert nv.load().g2048_abi_version() == 4


def test_invalid_arguments_return_einval_without_touching_a_device():
    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    assert lib.g2048_f32split_pack(None, 256, 256, 1.0, a, None) == -1
    assert lib.g2048_f32split_pack(a, 256, 512, 1.0, a, None) == -1          # K
    assert lib.g2048_f32split_pack(a, 512, 256, 1.0, a, None) == -1          # N
    assert lib.g2048_f32split_pack(a, 256, 256, 3.0, a, None) == -1          # scale not a power of two
    assert lib.g2048_f32split_pack(a, 256, 256, 1.0, a + 8, None) == -1      # alignment
    order = ("x", "ldx", "w", "bias", "y", "ldy", "resid", "gamma", "beta", "h", "T", "K", "N", "epi", "sx", "sw", "eps", "stream")
    base = dict(x=a, ldx=256, w=a, bias=a, y=a, ldy=256, resid=a, gamma=a, beta=a, h=a, T=4, K=256, N=256, epi=nv.F32SPLIT_ADD_LN,
                sx=1.0, sw=1.0, eps=1e-5, stream=None)
    gemm = lambda **k: lib.g2048_f32split_gemm(*[{**base, **k}[n] for n in order])
    assert gemm(x=None) == -1 and gemm(w=None) == -1 and gemm(bias=None) == -1 and gemm(y=None) == -1
    assert gemm(T=0) == -1 and gemm(K=128) == -1 and gemm(N=512) == -1 and gemm(epi=7) == -1
    assert gemm(N=768, ldy=768) == -1                       # row epilogues need N = 256
    assert gemm(resid=None) == -1 and gemm(gamma=None) == -1 and gemm(h=None) == -1
    assert gemm(ldx=128) == -1 and gemm(ldy=255) == -1 and gemm(ldx=258) == -1
    assert gemm(sx=0.0) == -1 and gemm(sw=1.5) == -1 and gemm(sx=float("inf")) == -1
    assert gemm(x=a + 4) == -1
    assert lib.g2048_attn_fwd_f32(None, a, 4, 8, 1.0, None) == -1
    assert lib.g2048_attn_fwd_f32(a, a, 0, 8, 1.0, None) == -1
    assert lib.g2048_attn_fwd_f32(a, a, 4, 0, 1.0, None) == -1
    assert lib.g2048_embed_ln_f32(None, a, a, a, a, 1e-5, a, a, 4, None) == -1
    assert lib.g2048_embed_ln_f32(a, a, a, a, a, 1e-5, a, a, 0, None) == -1
    assert lib.g2048_embed_ln_f32(a, a + 4, a, a, a, 1e-5, a, a, 4, None) == -1


def test_switch_stays_on_the_module_forward_on_a_cpu_agent():
    from src.ppo import PPOAgent
    from src.ppo.torch_action_wrapper import TorchActionFunction

    torch.manual_seed(0)
    agent = PPOAgent(reduction="cls", num_layers=1)
    fn = TorchActionFunction(agent, fp32_native=True)
    assert fn.fp32_native and fn._fused is None
    boards = torch.from_numpy(np.arange(32, dtype=np.uint8).reshape(2, 16) % 12)
    logits, values = fn.policy_fn(boards, None)
    want_l, want_v = agent(boards, None)
    assert torch.equal(logits, want_l.float()) and torch.equal(values, want_v.float().reshape(-1))
    assert TorchActionFunction(agent).fp32_native in (False, True)  # (the environment decides; see the parser test)


def test_environment_variable_parses_like_the_other_switches():
    from src.ppo.torch_action_wrapper import resolve_fp32_native

    for v in ("1", "true", "YES", " on "):
        assert resolve_fp32_native(None, {"G2048_ROLLOUT_FP32_NATIVE": v}) is True
    for v in ("", "0", "false", "no", "off", "2"):
        assert resolve_fp32_native(None, {"G2048_ROLLOUT_FP32_NATIVE": v}) is False
    assert resolve_fp32_native(None, {}) is False
    assert resolve_fp32_native(False, {"G2048_ROLLOUT_FP32_NATIVE": "1"}) is False
    assert resolve_fp32_native(True, {}) is True
