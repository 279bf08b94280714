"""Shared plumbing for the act_fn plug-ins: run the batched device kernel on un-batched host inputs."""
import os

import numpy as np
import torch

from ..env_definitions import BOARD_FLAT_DIM, OBS_DIM
from ..g2048 import native as nv

RNG_MODES = {"legacy": nv.RNG_LEGACY, "partitionable": nv.RNG_PARTITIONABLE, "0": 0, "1": 1}


def resolve_rng_mode(rng_mode=None) -> int:
    """The one reading of an rng mode (BatchRunner, every act_fn plug-in, the n-tuple trainer).  ``None`` asks G2048_RNG_MODE
    (default "partitionable"); a string is one of RNG_MODES, case-insensitive; an int passes through.  Any other spelling, given
    as the argument or in the environment, raises ``ValueError``: none silently means "partitionable"."""
    if rng_mode is None:
        rng_mode = os.environ.get("G2048_RNG_MODE", "partitionable")
    if isinstance(rng_mode, str):
        if rng_mode.lower() not in RNG_MODES:
            raise ValueError(f"unknown rng_mode {rng_mode!r}")
        return RNG_MODES[rng_mode.lower()]
    return int(rng_mode)


def device():
    if not torch.cuda.is_available():
        raise nv.NativeError("act_fn plug-ins run on the MI355X; no HIP device is visible and no CPU path exists")
    return torch.device("cuda", torch.cuda.current_device())


def mask_to_bits(mask) -> torch.Tensor:
    """bool [..., 4] (numpy or torch) -> u8 bitmask tensor [...] on the device."""
    m = torch.as_tensor(np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask)).to(torch.bool)
    if m.shape[-1] != 4:
        raise AssertionError(f"mask must have 4 entries, got shape {tuple(m.shape)}")
    w = torch.tensor([1, 2, 4, 8], dtype=torch.uint8)
    return (m.to(torch.uint8) * w).sum(-1).to(torch.uint8).reshape(-1).to(device())


def keys_tensor(rng_key) -> torch.Tensor:
    """key words u32 [2] or [B, 2] -> device key tensor [B, 2]."""
    k = np.asarray(rng_key.cpu() if isinstance(rng_key, torch.Tensor) else rng_key)
    return nv.keys_from_numpy(k.reshape(-1, 2), device())


def obs_rows(obs):
    """One-hot observation [..., 4, 4, 31] (numpy or torch) -> (f32 [n, 16, 31] on the host, whether it had batch dimensions)."""
    obs_t = torch.as_tensor(np.asarray(obs.cpu() if isinstance(obs, torch.Tensor) else obs))
    return obs_t.reshape(-1, BOARD_FLAT_DIM, OBS_DIM).float(), obs_t.ndim > 3


def act_on_logits(rng_key, logits, values, mask, use_mask: bool, sample: bool, rng_mode, batched: bool):
    """The tail of the un-batched plug-in protocol: ``g2048_act_logits`` on logits [n, 4] -> (action, log_prob, value) as numpy
    arrays if ``batched``, as numpy scalars of row 0 otherwise.  ``rng_mode`` goes through ``resolve_rng_mode``."""
    dev = device()
    bits = mask_to_bits(mask)
    keys = keys_tensor(rng_key)
    n = bits.numel()
    actions = torch.empty(n, dtype=torch.int32, device=dev)
    logp = torch.empty(n, dtype=torch.float32, device=dev)
    nv.act_logits(keys, logits.float().to(dev).contiguous(), bits, use_mask, sample, actions, logp, resolve_rng_mode(rng_mode))
    a, lp, v = actions.cpu().numpy(), logp.cpu().numpy(), values.float().reshape(-1).cpu().numpy()
    if batched:
        return a, lp, v
    return np.int32(a[0]), np.float32(lp[0]), np.float32(v[0])
