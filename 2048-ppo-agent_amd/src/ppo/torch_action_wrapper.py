"""Policy -> act_fn bridge (API of the reference src/ppo/torch_action_wrapper.py:10-104).

The reference converts the torch agent to JAX (torch2jax) so it can be vmapped next to the Pgx env.  Here the
env lives on the GPU, so the agent simply runs batched in PyTorch-ROCm on the packed boards and the tail of
``__call__`` (clamp, categorical draw from the JAX-compatible key stream, log-softmax pick) is fused with the
env step in ``g2048_policy_step`` / available stand-alone as ``g2048_act_logits``.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from ..actions import _common as C
from ..g2048 import native as nv
from .capture import capture as capture_graph


def resolve_fp32_native(fp32_native=None, environ=None) -> bool:
    """An explicit argument wins; else G2048_ROLLOUT_FP32_NATIVE=1/true/yes/on (parsed like G2048_ROLLOUT_FP32); default off."""
    if fp32_native is not None:
        return bool(fp32_native)
    environ = os.environ if environ is None else environ
    return environ.get("G2048_ROLLOUT_FP32_NATIVE", "0").strip().lower() in ("1", "true", "yes", "on")


SYMMETRY_MODES = ("none", "canonical", "ensemble")  # exclusive: canonical + ensemble would average eight copies of one row


def resolve_symmetry(symmetry=None, environ=None) -> str:
    """An explicit argument wins; else G2048_SYMMETRY; default "none".  -> one of SYMMETRY_MODES; anything else raises."""
    if symmetry is None:
        environ = os.environ if environ is None else environ
        symmetry = environ.get("G2048_SYMMETRY", "none").strip().lower() or "none"
    if symmetry not in SYMMETRY_MODES:
        raise ValueError(f"symmetry must be one of {SYMMETRY_MODES} (or None: ask G2048_SYMMETRY), got {symmetry!r}")
    return symmetry


class TorchActionFunction:
    """Wrap an actor-critic ``agent`` as an ``act_fn`` plug-in for BatchRunner.

    Parameters mirror the reference: ``agent``, ``use_mask`` (apply the legal-action mask to the logits),
    ``sample_actions`` (categorical sample vs argmax), ``device`` (where the agent runs).  Extra:
    ``amp_dtype`` runs the rollout forward under autocast (the reference rolls out in fp32) -- for bfloat16 and a
    PPOAgent of the reference's default shape ("cls" or "mean" reduction) the encoder then runs in the fused MFMA kernel unless
    ``use_fused=False``; ``sync_every`` is how many lock-steps are enqueued between polls of the device-side
    live-env counter; ``fp32_native`` sends an fp32 rollout (``amp_dtype`` None) of such a PPOAgent on a HIP device through the
    split-fp16 kernels (``fused_policy.FusedPolicyF32``: f32-grade results on the f16 matrix cores) - ``None`` asks
    G2048_ROLLOUT_FP32_NATIVE (default off); anywhere else the switch does nothing and the module forward runs.
    ``symmetry="canonical"`` (``None`` asks G2048_SYMMETRY, default "none") puts every forward into the canonical frame: the
    boards are turned into the lexicographically largest of their eight dihedral views (``g2048_sym_canon``), the forward above
    runs unchanged on those, and the four logits are turned back into the env's frame (``g2048_sym_logits``).  The policy is then
    exactly equivariant and the value exactly invariant under the symmetries of the board, for one forward; the env, its key
    stream and the trajectory stay in the env's frame.  Train and evaluate an agent in the same mode.
    ``symmetry="ensemble"`` is for play and needs no retraining: the forward above runs unchanged on all eight views of every board
    (``g2048_sym_views``, 8 B rows) and ``g2048_sym_fold`` takes the mean over the views, the logits at the action that does in
    the view what ``a`` does in the env's frame, in an order that depends on the eight addends as a multiset only.  Any agent
    whose forward treats a row independently of its slot thereby becomes exactly equivariant in policy and exactly invariant in
    value, at eight times the forward rows.  ``PPOTrainer`` refuses the mode.
    Side effect as in the reference: ``agent`` is moved to ``device`` and put in eval mode.
    """

    def __init__(self, agent, use_mask: bool = False, sample_actions: bool = True,
                 device: torch.device = torch.device("cpu"), amp_dtype: Optional[torch.dtype] = None,
                 sync_every: int = 8, rng_mode=None, use_fused: Optional[bool] = None, graph_cache: Optional[dict] = None,
                 fp32_native: Optional[bool] = None, symmetry: Optional[str] = None):
        self.symmetry = resolve_symmetry(symmetry)  # (first: an unknown mode is refused before the agent is touched)
        self.agent = agent.to(device).eval()
        self.use_mask = use_mask
        self.sample_actions = sample_actions
        self.device = device
        self.amp_dtype = amp_dtype
        self.sync_every = sync_every
        self.rng_mode = rng_mode
        # bf16 rollouts of a default-shape PPOAgent go through the fused MFMA encoder kernel (csrc/g2048_policy.hip)
        self._fused = None
        if amp_dtype == torch.bfloat16 and use_fused is not False:
            from . import fused_policy

            if fused_policy.supports(self.agent) or fused_policy.supports_mean(self.agent):
                self._fused = fused_policy.FusedPolicy(self.agent)
        # fp32 rollouts of the same agents: the split-fp16 forward (csrc/g2048_f32split.hip), opt-in
        self.fp32_native = resolve_fp32_native(fp32_native)
        if amp_dtype is None and self.fp32_native:
            from . import fused_policy

            if fused_policy.supports(self.agent) or fused_policy.supports_mean(self.agent):
                self._fused = fused_policy.FusedPolicyF32(self.agent)
        # a cheap policy (the MLP of BASELINE configs[1]: ~15 launches of microseconds per lock-step) is launch-bound in eager
        # mode: with a ``graph_cache`` (owned by the caller, it outlives this object) the forward over ALL boards of the batch is
        # replayed from a hipGraph and the engine skips the live-board compaction (``compact``), whose gathers cost more than
        # the forward they would save
        self._graph_cache = graph_cache if (self._fused is None and torch.device(device).type == "cuda") else None
        self.compact = self._graph_cache is None
        self._agent_params = dict(self.agent.named_parameters())
        self._agent_buffers = dict(self.agent.named_buffers())
        self._agent_state = {**self._agent_params, **self._agent_buffers}

    # batched device path used by the rollout engine: raw actor logits (masking happens in the kernel)
    @torch.no_grad()
    def policy_fn(self, boards: torch.Tensor, masks: torch.Tensor):
        """boards u8 [B, 16], masks u8 [B] or None (unused here) -> (logits f32 [B, 4], values f32 [B])."""
        if self.symmetry == "canonical":
            canon, frame = self._canonical(boards)
            logits, values = self._policy(canon)
            logits = logits.contiguous()
            if logits.data_ptr() % 16:  # (a view into a larger tensor: the kernel moves 16-byte rows)
                logits = logits.clone()
            if logits.shape[0]:
                nv.sym_logits(logits, frame)  # in place: nothing keeps the forward's output in the canonical frame
            return logits, values
        if self.symmetry == "ensemble":
            return self._ensemble(boards, want_logits=True)
        return self._policy(boards)

    policy_fn.needs_masks = False  # (RolloutEngine.rollout_policy: no per-lock-step gather of the masks for this policy)

    @staticmethod
    def _canonical(boards: torch.Tensor, with_frame: bool = True):
        """boards u8 [n, 16] -> (their canonical views (a new tensor), frame u8 [n] or None)."""
        boards = boards.contiguous()
        canon = torch.empty_like(boards)
        frame = torch.empty(boards.shape[0], dtype=torch.uint8, device=boards.device) if with_frame else None
        if boards.shape[0]:
            nv.sym_canon(boards, canon, frame=frame)
        return canon, frame

    def _ensemble(self, boards: torch.Tensor, want_logits: bool = True):
        """boards u8 [n, 16] -> (logits f32 [n, 4] in the env's frame or None, values f32 [n]): ``self._policy`` on the 8 n view
        rows, folded.  The fold reads the forward's outputs where they lie (a replayed graph's
        static outputs included) and writes new tensors."""
        boards = boards.contiguous()
        n, dev = boards.shape[0], boards.device
        out_logits = torch.empty((n, 4), dtype=torch.float32, device=dev) if want_logits else None
        out_values = torch.empty(n, dtype=torch.float32, device=dev)
        if n == 0:
            return out_logits, out_values
        views = torch.empty((8 * n, 16), dtype=torch.uint8, device=dev)
        nv.sym_views(boards, views)
        logits, values = self._policy(views)
        values = values.to(torch.float32).reshape(-1).contiguous()
        if want_logits:
            logits = logits.to(torch.float32).contiguous()
            if logits.data_ptr() % 16:  # (a view into a larger tensor: the kernel loads 16-byte rows)
                logits = logits.clone()
        nv.sym_fold(logits if want_logits else None, values, out_logits, out_values)
        return out_logits, out_values

    def _policy(self, boards: torch.Tensor):
        """The forward as it is without a symmetry mode: fused kernel, replayed graph or module, whichever applies."""
        agent_dev = next(self.agent.parameters()).device
        if self._fused is not None and boards.device == agent_dev:
            return self._fused(boards)
        if self._graph_cache is not None and boards.device == agent_dev:
            out = self._graphed(boards)
            if out is not None:
                return out
        return self._forward(boards, agent_dev)

    def _forward(self, boards, agent_dev):
        x = boards if boards.device == agent_dev else boards.to(agent_dev)
        if self.amp_dtype is not None and agent_dev.type == "cuda":
            with torch.autocast(device_type="cuda", dtype=self.amp_dtype):
                logits, values = self.agent(x, None)
        else:
            logits, values = self.agent(x, None)
        return logits.float().to(boards.device), values.float().reshape(-1).to(boards.device)

    def _graphed(self, boards: torch.Tensor):
        """The forward replayed from a hipGraph (captured once per batch shape; the parameters are read in place, so later
        optimiser steps are seen).  None: capture is not possible for this agent (remembered in the cache), run eagerly."""
        prepare = getattr(self.agent, "prepare_rollout", None)
        key = (tuple(boards.shape), boards.dtype, self.amp_dtype, next(self.agent.parameters()).data_ptr())
        entry = self._graph_cache.get(key, False)
        if entry is False:
            entry = None
            try:
                if prepare is not None:
                    prepare()  # (before the capture: the refresh must not become part of the graph)
                static_in = torch.empty_like(boards)
                static_in.copy_(boards)
                side = torch.cuda.Stream(device=boards.device)
                side.wait_stream(torch.cuda.current_stream(boards.device))
                with torch.cuda.stream(side):
                    for _ in range(2):
                        self._forward(static_in, boards.device)
                torch.cuda.current_stream(boards.device).wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with capture_graph(graph):  # thread-local error mode + no garbage collection while capturing (capture.py)
                    out = self._forward(static_in, boards.device)
                entry = (graph, static_in, out)
            except Exception as e:  # not capturable: eager from now on (the reason stays visible in the cache)
                self._graph_cache["fallback"] = repr(e)
            self._graph_cache[key] = entry
        if entry is None:
            return None
        graph, static_in, out = entry
        if prepare is not None:
            prepare()
        static_in.copy_(boards)
        graph.replay()
        return out

    @torch.no_grad()
    def __call__(self, rng_key, obs, mask):
        """Un-batched plug-in protocol: ``(rng_key[2], obs[4,4,31], mask[4]) -> (action, log_prob, value)``.
        Leading batch dimensions are accepted.  The draw and the log-prob come from ``g2048_act_logits`` (the tail shared with
        the score players, ``actions/_common.act_on_logits``); ``rng_mode`` is read by ``resolve_rng_mode``, so a string works
        here as it does in ``BatchRunner`` and an unknown one raises ``ValueError``."""
        obs_t, batched = C.obs_rows(obs)
        dev = C.device()
        if self.symmetry != "none":  # the one-hot observation is decoded to packed boards and goes down policy_fn
            logits, values = self.policy_fn(obs_t.argmax(dim=-1).to(torch.uint8).to(dev), None)
        else:
            agent_dev = next(self.agent.parameters()).device
            logits, values = self.agent(obs_t.to(agent_dev), None)
        return C.act_on_logits(rng_key, logits, values, mask, self.use_mask, self.sample_actions, self.rng_mode, batched)
