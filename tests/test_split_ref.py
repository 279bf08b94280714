"""The CPU model behind the fp32 rollout forward on split-fp16 products (tests/split_ref.py), pinned as ORDERINGS: which split
reaches the 1e-5 the eager fp32 forward is held to on the reference's ``default/*`` vectors, and which does not.  CPU only."""
import copy
import os

import numpy as np
import pytest
import torch

import split_ref as sr
from test_host_logic import default_shape_agent

REF = np.load(os.path.join(os.path.dirname(__file__), "golden", "torch_reference.npz"))
BOARDS = REF["default/boards"]


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.fixture(scope="module")
def agent():
    return default_shape_agent(dropout=0.0).eval()


@pytest.mark.parametrize("reduction", ["cls", "mean"])
def test_float64_forward_agrees_with_the_module(agent, reduction):
    """The yardstick itself: the written-out float64 forward vs the module's own fp32 forward, 1e-5."""
    a = copy.deepcopy(agent)
    a.reduction = reduction
    with torch.no_grad():
        tb = torch.from_numpy(BOARDS)
        feats = a.features(tb).numpy()
        logits, values = a(tb, None)
    f64 = sr.forward(sr.state_dict_numpy(a), BOARDS, reduction)
    assert _err(feats, f64[0]) < 1e-5 and _err(logits.numpy(), f64[1]) < 1e-5 and _err(values.numpy().reshape(-1), f64[2]) < 1e-5
    if reduction == "cls":  # and against the reference's own outputs
        assert _err(f64[1], REF["default/logits"]) < 1e-5 and _err(f64[0], REF["default/features"]) < 3e-5


@pytest.mark.parametrize("flush", [False, True])
def test_fp16_three_products_at_the_kernels_scales_reach_the_fixture(agent, flush):
    """hi hi + hi lo + lo hi in fp16 at the scales FusedPolicyF32 uses: within the bounds test_default_shape_agent_on_every_device_path
    puts on the eager fp32 forward, whether or not the matrix core keeps fp16 subnormals."""
    got = sr.forward(sr.state_dict_numpy(agent), BOARDS, "cls", product=sr.kernel_products(agent, flush=flush), dtype=np.float32)
    errs = (_err(got[0], REF["default/features"]), _err(got[1], REF["default/logits"]), _err(got[2], REF["default/values"].reshape(-1)))
    print("features / logits / values vs the fixture:", errs)
    assert errs[0] <= 3e-5 and errs[1] <= 1e-5 and errs[2] <= 1e-5


def test_bf16_three_products_and_unscaled_flushed_fp16_do_not(agent):
    sd = sr.state_dict_numpy(agent)
    bf = sr.forward(sd, BOARDS, "cls", product=sr.uniform_products("bf16"), dtype=np.float32)
    assert _err(bf[1], REF["default/logits"]) > 1e-5
    fl = sr.forward(sd, BOARDS, "cls", product=sr.uniform_products("fp16", flush=True), dtype=np.float32)
    assert _err(fl[1], REF["default/logits"]) > 1e-5


@pytest.mark.parametrize("k", [-12, -6, 6, 12])
def test_scales_follow_a_rescaled_hidden_layer_without_a_fallback(agent, k):
    """linear1 * 2^k, linear2 / 2^k: the bounds the scales come from move with the weights, so the split model of the rescaled
    agent passes the whole-forward acceptance against ITS float64 forward, with subnormals flushed (the pessimistic reading)."""
    a = sr.rescale_hidden(copy.deepcopy(agent), k)
    sd = sr.state_dict_numpy(a)
    f64 = sr.forward(sd, BOARDS, "cls")
    f32 = sr.forward(sd, BOARDS, "cls", dtype=np.float32)
    got = sr.forward(sd, BOARDS, "cls", product=sr.kernel_products(a, flush=True), dtype=np.float32)
    for i in (1, 2):
        assert sr.accept(_err(got[i], f64[i]), _err(f32[i], f64[i])), (k, i, _err(got[i], f64[i]), _err(f32[i], f64[i]))


def test_scales_are_powers_of_two_and_keep_every_operand_finite(agent):
    from src.ppo.fused_policy import F16_TOP, f32_split_scales

    sd = sr.state_dict_numpy(agent)
    scales = f32_split_scales(agent)
    seen = {}

    def spy(x, w, name):
        seen[name] = (float(np.abs(x).max()), float(np.abs(w).max()))
        return x @ w.T

    sr.forward(sd, BOARDS, "cls", product=spy)
    keys = {"self_attn.in_proj": ("h1", "wqkv"), "self_attn.out_proj": ("a", "wo"), "linear1": ("h2", "w1"), "linear2": ("f", "w2")}
    for i, s in enumerate(scales):
        for v in s.values():
            assert np.frexp(v)[0] == 0.5
        for name, (kx, kw) in keys.items():
            mx, mw = seen[f"transformer.encoder.layers.{i}.{name}"]
            assert mx * s[kx] <= F16_TOP and mw * s[kw] <= F16_TOP
            assert mx * s[kx] >= 2.0 ** 6, (name, mx * s[kx])  # the bound is not so loose that typical operands near the floor
