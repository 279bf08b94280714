"""Imitation learning of a ``PPOAgent`` from a score-playing teacher (no reference counterpart: the reference only trains by PPO).

    collect:  always-live envs on the engine's key chain; per lock-step the teacher scores every board (``policy_fn`` of a
              ``QPlayer``, first of all ``NTupleActionFunction``), a fixed share ``beta`` of the envs plays the teacher's masked
              argmax and the rest the student's (DAgger: the student visits its own states, the teacher labels them), and
              (board, legal mask, q, v) go into a device ring.  Nothing is read back.
    update:   minibatches drawn on the device -> ``g2048_distill_gather`` -> the agent's forward under autocast (the fused update
              nodes ``PPOTrainer`` reaches) -> ``g2048_distill_loss``: cross-entropy to the teacher, its means and its gradients in
              two launches -> backward -> global-norm clip -> optimiser step.  Eager: no hipGraph here.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional

import torch
from torch.amp import GradScaler, autocast

from ..actions import _common as C
from ..g2048 import native as nv
from ..g2048.engine import seed_key
from ..optim import configure_bert_optimizers
from ..optim.eager_step import eager_step, loss_scale
from .ntuple import NTupleActionFunction, NTupleNetwork
from .torch_action_wrapper import TorchActionFunction

# run/train_to_2048.py's optimiser settings: what the flagship script trains the same model shape with
DEFAULT_OPTIM = dict(opt_name="adamw", max_lr=4e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, warmup_steps_ratio=0.025,
                     scheduler_names=["constant", "constant"], blacklist_weight_modules=["norm", "embedding"])
MAX_GRAD_NORM = 0.5
OPTIM_STEPS = 500000  # the schedule's length (constant after the warm-up), as train_to_2048.py passes it


class _FusedDistillLoss(torch.autograd.Function):
    """The imitation loss in two HIP launches (``g2048_distill_loss``): forward, the logged means and the gradient.

    -> (sums f32 [5] = mean cross-entropy, value loss, entropy loss (-H), TOTAL loss, agreement; new_log_probs [M] = the student's
    log-probability of the teacher's move).  Shaped like ``_FusedPPOLoss``: only ``sums[3]`` is differentiable and backward hands
    on the gradients the kernel already made, multiplied by ``grad_scale`` (the GradScaler's device scalar) inside the kernel when
    one is given.  ``values`` and ``value_target`` are None together: no critic term, no gradient for the critic."""

    @staticmethod
    def forward(ctx, logits, values, mask_bits, teacher_q, value_target, tau, c_value, c_entropy, grad_scale=None, running=None,
                workspace=None):
        new_lp, sums, dlogits, dvalues = nv.distill_loss(logits.contiguous(), None if values is None else values.contiguous(),
                                                         mask_bits, teacher_q, value_target, tau, c_value, c_entropy, grad_scale,
                                                         running, workspace)
        ctx.has_values = dvalues is not None
        ctx.save_for_backward(*((dlogits, dvalues) if ctx.has_values else (dlogits,)))
        ctx.prescaled = grad_scale is not None
        ctx.mark_non_differentiable(new_lp)
        ctx.set_materialize_grads(False)
        return sums, new_lp

    @staticmethod
    def backward(ctx, g_sums, _g_new_lp):
        dlogits = ctx.saved_tensors[0]
        dvalues = ctx.saved_tensors[1] if ctx.has_values else None
        if not ctx.prescaled:
            g = g_sums[3].to(dlogits.dtype)
            dlogits = dlogits * g
            dvalues = None if dvalues is None else dvalues * g.to(dvalues.dtype)
        return (dlogits, dvalues) + (None,) * 9


def _finite_non_negative(x, name: str) -> float:
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite non-negative number, got {x!r}") from None
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be a finite non-negative number, got {x!r}")
    return v


class DistillTrainer:
    """Cross-entropy distillation of ``teacher`` into ``agent`` on ``num_envs`` always-live boards.

    ``teacher``: anything with ``policy_fn(boards u8 [B, 16], masks u8 [B]) -> (q f32 [B, 4], v f32 [B])`` - an
    ``NTupleActionFunction`` at any ``plies``, any ``QPlayer``; an ``NTupleNetwork`` is wrapped at ``plies=0``.  The first
    ``ceil(beta * num_envs)`` envs play the teacher's masked argmax, the others the student's (``beta=1``: behaviour cloning,
    ``beta=0``: only the student's own states are labelled); which env does which is fixed, no extra random numbers are drawn.  The
    ring holds ``capacity`` rows: boards, legal masks, the teacher's q and ``v * value_scale``.  ``tau=0`` trains on the teacher's
    move (one-hot), ``tau > 0`` on softmax(q / tau) over the legal moves.  ``value_coef=0`` (default) leaves the critic untouched;
    ``value_coef > 0`` also regresses it to the scaled teacher value.  ``optimizer_param_dict``: ``configure_bert_optimizers``
    settings, by default those of run/train_to_2048.py.  Bad settings raise ``ValueError`` before any device is touched.
    """

    def __init__(self, agent, teacher, num_envs: int, capacity: int, batch_size: int = 4096, tau: float = 0.0, beta: float = 0.5,
                 value_coef: float = 0.0, value_scale: float = 1.0, entropy_coef: float = 0.0, optimizer_param_dict: Optional[dict] = None,
                 mixed_precision: Optional[str] = "bfloat16", seed: int = 0, rng_mode=None, device=None):
        self.tau = _finite_non_negative(tau, "tau")
        self.value_coef = _finite_non_negative(value_coef, "value_coef")
        try:
            self.beta = float(beta)
        except (TypeError, ValueError):
            raise ValueError(f"beta must be in [0, 1], got {beta!r}") from None
        if not 0.0 <= self.beta <= 1.0:
            raise ValueError(f"beta must be in [0, 1], got {beta!r}")
        if int(num_envs) < 1:
            raise ValueError(f"num_envs must be positive, got {num_envs!r}")
        if int(batch_size) < 1 or int(batch_size) > nv.CONSTANTS["G2048_PPO_LOSS_MAX_BATCH"]:
            raise ValueError(f"batch_size must be in 1 .. {nv.CONSTANTS['G2048_PPO_LOSS_MAX_BATCH']}, got {batch_size!r}")
        if int(capacity) < int(batch_size):
            raise ValueError(f"capacity ({capacity!r}) must be at least batch_size ({batch_size!r})")
        if int(capacity) < int(num_envs):
            raise ValueError(f"capacity ({capacity!r}) must hold one lock-step of num_envs ({num_envs!r}) rows")
        if getattr(agent, "action_dim", None) != 4:
            raise ValueError(f"the agent must have action_dim 4, got {getattr(agent, 'action_dim', None)!r}")
        if mixed_precision not in (None, "float16", "bfloat16"):
            raise ValueError(f"mixed_precision must be None, 'float16' or 'bfloat16', got {mixed_precision!r}")
        if not (math.isfinite(float(value_scale)) and math.isfinite(float(entropy_coef))):
            raise ValueError(f"value_scale and entropy_coef must be finite, got {value_scale!r}, {entropy_coef!r}")
        if isinstance(teacher, NTupleNetwork):
            teacher = NTupleActionFunction(teacher, plies=0)
        if not callable(getattr(teacher, "policy_fn", None)):
            raise ValueError(f"teacher must be an NTupleNetwork or have policy_fn(boards, masks) -> (q, v), got {type(teacher).__name__}")
        self.teacher = teacher
        self.num_envs, self.capacity, self.batch_size = int(num_envs), int(capacity), int(batch_size)
        self.value_scale, self.entropy_coef = float(value_scale), float(entropy_coef)
        self.n_teacher = self._teacher_envs(self.beta)
        self.rng_mode = C.resolve_rng_mode(rng_mode)
        self.seed = int(seed)

        self.device = dev = C.device() if device is None else torch.device(device)
        self.agent = agent.to(dev)
        self.mixed_precision = mixed_precision
        self.use_amp = mixed_precision is not None and dev.type == "cuda"
        self.amp_dtype = (torch.float16 if mixed_precision == "float16" else torch.bfloat16) if self.use_amp else None
        self.scaler = GradScaler() if self.use_amp else None
        opt = configure_bert_optimizers(self.agent, steps=OPTIM_STEPS, **dict(DEFAULT_OPTIM if optimizer_param_dict is None
                                                                              else optimizer_param_dict))
        self.optimizer, self.lr_scheduler = opt["optimizer"], opt["lr_scheduler"]["scheduler"]
        # the student's rollout forward: the no-grad forward TorchActionFunction uses (the fused encoder kernel for bf16)
        self._student = TorchActionFunction(self.agent, use_mask=True, sample_actions=False, device=dev, amp_dtype=self.amp_dtype,
                                            rng_mode=rng_mode, symmetry="none")
        self._critic_params = list(self.agent.critic.parameters()) if hasattr(self.agent, "critic") else []

        u8, f32 = torch.uint8, torch.float32
        B, N, M = self.num_envs, self.capacity, self.batch_size
        self.key = seed_key(self.seed)
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(self.seed)
        self.boards = torch.empty((B, 16), dtype=u8, device=dev)
        self.masks = torch.empty(B, dtype=u8, device=dev)
        self.ep_len = torch.empty(B, dtype=torch.int32, device=dev)
        self._done = torch.empty(B, dtype=u8, device=dev)
        self._act = torch.empty((B, 4), dtype=f32, device=dev)
        self._tr = dict(boards=torch.empty((1, B, 16), dtype=u8, device=dev), meta=torch.empty((1, B), dtype=u8, device=dev),
                        rewards=torch.empty((1, B), dtype=f32, device=dev), logp=torch.empty((1, B), dtype=f32, device=dev),
                        values=torch.empty((1, B), dtype=f32, device=dev))
        self.ring = dict(boards=torch.zeros((N, 16), dtype=u8, device=dev), masks=torch.zeros(N, dtype=u8, device=dev),
                         q=torch.zeros((N, 4), dtype=f32, device=dev), vt=torch.zeros(N, dtype=f32, device=dev))
        self._mb = dict(obs=torch.empty((M, 16), dtype=u8, device=dev), masks=torch.empty(M, dtype=u8, device=dev),
                        q=torch.empty((M, 4), dtype=f32, device=dev), vt=torch.empty(M, dtype=f32, device=dev))
        self._running = torch.zeros(5, dtype=torch.float64, device=dev)
        self._sel = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device=dev)
        self._workspace = None  # allocated at the first update (the size comes from the library)
        # the largest log2 tile seen on a board the student played (u8 [] on the device)
        self.student_top = torch.zeros((), dtype=u8, device=dev)
        self._started = False
        self.pos = 0          # the ring's write position
        self.filled = 0       # valid rows in the ring
        self.rows = 0         # rows collected over the trainer's lifetime
        self.lock_steps = 0
        self.updates = 0

    def _teacher_envs(self, beta: float) -> int:
        """ceil(beta * num_envs); the small slack keeps a product such as 0.7 * 10 = 7.000000000000001 at 7."""
        return min(self.num_envs, int(math.ceil(beta * self.num_envs - 1e-9)))

    # ------------------------------------------------------------------ collect
    def _ring_write(self, name: str, src: torch.Tensor):
        ring, pos, B, N = self.ring[name], self.pos, self.num_envs, self.capacity
        head = min(B, N - pos)
        ring[pos:pos + head].copy_(src[:head])
        if head < B:
            ring[:B - head].copy_(src[head:])

    @torch.no_grad()
    def collect(self, lock_steps: int) -> int:
        """``lock_steps`` lock-steps of all envs into the ring -> the number of rows added."""
        T, B, tr, nt = int(lock_steps), self.num_envs, self._tr, self.n_teacher
        if T < 1:
            raise ValueError(f"lock_steps must be positive, got {lock_steps!r}")
        self.agent.eval()
        if not self._started:
            self.key, sub = nv.chain_keys(self.key, 1, self.rng_mode)
            nv.reset_fused(sub[0], self.boards, self.masks, self._done, self.ep_len, B, 0, self.rng_mode)
            self._started = True
        self.key, subs = nv.chain_keys(self.key, 2 * T, self.rng_mode)
        for t in range(T):
            q, v = self.teacher.policy_fn(self.boards, self.masks)
            q, v = q.float().contiguous(), v.float().reshape(-1).contiguous()
            if nt == B:
                act = q
            else:
                logits, _ = self._student.policy_fn(self.boards[nt:], None)
                act = self._act
                act[:nt].copy_(q[:nt])
                act[nt:].copy_(logits)
            nv.policy_step_autoreset(subs[2 * t], subs[2 * t + 1], act, v, True, False, 0, self.boards, self.masks, self.ep_len,
                                     tr["boards"], tr["meta"], tr["rewards"], tr["logp"], tr["values"], B, 0, self.rng_mode)
            # the trajectory row holds the boards before the step and meta = action | mask_before << 2 | done_after << 6
            self._ring_write("boards", tr["boards"][0])
            self._ring_write("masks", (tr["meta"][0] >> 2) & 15)
            self._ring_write("q", q)
            self._ring_write("vt", v * self.value_scale)
            if nt < B:
                torch.maximum(self.student_top, tr["boards"][0][nt:].max(), out=self.student_top)
            self.pos = (self.pos + B) % self.capacity
            self.filled = min(self.capacity, self.filled + B)
        self.rows += T * B
        self.lock_steps += T
        return T * B

    # ------------------------------------------------------------------ update
    def _loss_backward(self, batch: dict):
        """Forward + loss + (scaled) backward of one gathered minibatch -> sums f32 [5], detached."""
        ctx = autocast(device_type="cuda", dtype=self.amp_dtype) if self.use_amp else contextlib.nullcontext()
        with_v = self.value_coef > 0.0
        with ctx:
            logits, values = self.agent(batch["obs"], None)
            scale = loss_scale(self.scaler, self.device)  # the kernel applies the loss scale to its gradients
            sums, _ = _FusedDistillLoss.apply(logits, values.reshape(-1) if with_v else None, batch["masks"], batch["q"],
                                              batch["vt"] if with_v else None, self.tau, self.value_coef, self.entropy_coef, scale,
                                              self._running, self._workspace)
        self.optimizer.zero_grad(set_to_none=True)
        sums.backward(self._sel)
        if not with_v:  # the critic is not part of this loss: no step, no weight decay on it
            for p in self._critic_params:
                p.grad = None
        return sums.detach()

    def update(self, minibatches: int) -> torch.Tensor:
        """``minibatches`` optimiser steps on minibatches drawn uniformly (with replacement) from the ring's valid rows -> the five
        means of the last minibatch (f32 [5], device); their running sums are in ``train``'s result."""
        K, M = int(minibatches), self.batch_size
        if K < 1:
            raise ValueError(f"minibatches must be positive, got {minibatches!r}")
        if self.filled < 1:
            raise ValueError("update() before collect(): the ring is empty")
        if self._workspace is None:
            self._workspace = torch.empty(nv.distill_loss_workspace_floats(M), dtype=torch.float32, device=self.device)
        self.agent.train()
        ring, with_v = self.ring, self.value_coef > 0.0
        sums = None
        for _ in range(K):
            idx = torch.randint(0, self.filled, (M,), generator=self._gen, device=self.device, dtype=torch.int64)
            nv.distill_gather(idx, ring["boards"], ring["masks"], ring["q"], ring["vt"] if with_v else None,
                              out=self._mb if with_v else dict(self._mb, vt=None))
            sums = self._loss_backward(self._mb)
            eager_step(self.optimizer, self.scaler, self.agent.parameters(), MAX_GRAD_NORM, self.device)
            self.lr_scheduler.step()
            self.updates += 1
        return sums

    def train(self, iterations: int, collect_steps: int, minibatches: int) -> dict:
        """``iterations`` x (``collect(collect_steps)``, ``update(minibatches)``) -> {"ce": f64 [], "agreement": f64 [] (means over
        all minibatches of the call), "rows": i64 [] rows collected in the call}, device tensors: nothing is read back."""
        if int(iterations) < 1:
            raise ValueError(f"iterations must be positive, got {iterations!r}")
        self._running.zero_()
        rows = 0
        for _ in range(int(iterations)):
            rows += self.collect(collect_steps)
            self.update(minibatches)
        mean = self._running / float(int(iterations) * int(minibatches))
        return {"ce": mean[0].clone(), "agreement": mean[4].clone(), "rows": torch.tensor(rows, dtype=torch.int64, device=self.device)}

    @torch.no_grad()
    def score(self, other: Optional["DistillTrainer"] = None) -> dict:
        """The agent as it plays (the rollout forward, eval mode) on the valid rows of ``other``'s ring (default: its own) ->
        {"ce": f32 [], "agreement": f32 []}, device tensors: cross-entropy to and agreement with the labels stored there, at this
        trainer's ``tau``.  A held-out measurement when ``other`` collected with another seed."""
        src = self if other is None else other
        n = src.filled
        if n < 1:
            raise ValueError("score() on an empty ring")
        self.agent.eval()
        ce = torch.zeros((), dtype=torch.float32, device=self.device)
        agree = torch.zeros((), dtype=torch.float32, device=self.device)
        step = nv.CONSTANTS["G2048_PPO_LOSS_MAX_BATCH"]
        for s in range(0, n, step):
            e = min(n, s + step)
            logits, _ = self._student.policy_fn(src.ring["boards"][s:e], None)
            _, sums, _, _ = nv.distill_loss(logits.float().contiguous(), None, src.ring["masks"][s:e], src.ring["q"][s:e], None, self.tau,
                                            0.0, 0.0)
            ce += sums[0] * ((e - s) / n)
            agree += sums[4] * ((e - s) / n)
        return {"ce": ce, "agreement": agree}

    # ------------------------------------------------------------------ state
    SETTINGS =("num_envs", "capacity", "batch_size", "tau", "beta", "value_coef", "value_scale", "entropy_coef", "seed")
    COUNTS = ("lock_steps", "updates", "rows")

    def state_dict(self) -> dict:
        """The trainer's settings and step counts.  The agent and the optimiser are saved by their own means
        (``agent.state_dict()``, ``trainer.optimizer.state_dict()``); the ring and the envs start afresh."""
        return {k: getattr(self, k) for k in self.SETTINGS + self.COUNTS}

    def load_state_dict(self, state: dict) -> None:
        """Takes the loss settings and the counts; ``ValueError`` (nothing changed) for a state of another ``num_envs``, ``capacity``
        or ``batch_size`` (the buffers are sized by them), a missing key or a bad value."""
        missing = [k for k in self.SETTINGS + self.COUNTS if k not in state]
        if missing:
            raise ValueError(f"the state lacks {missing}")
        for k in ("num_envs", "capacity", "batch_size"):
            if int(state[k]) != getattr(self, k):
                raise ValueError(f"the state is of {k}={state[k]!r}, the trainer's is {getattr(self, k)}")
        tau, vc = _finite_non_negative(state["tau"], "tau"), _finite_non_negative(state["value_coef"], "value_coef")
        beta = float(state["beta"])
        if not 0.0 <= beta <= 1.0:
            raise ValueError(f"beta must be in [0, 1], got {state['beta']!r}")
        counts = {k: int(state[k]) for k in self.COUNTS}
        if min(counts.values()) < 0:
            raise ValueError(f"negative counts: {counts}")
        self.tau, self.value_coef, self.beta = tau, vc, beta
        self.n_teacher = self._teacher_envs(beta)
        self.value_scale, self.entropy_coef = float(state["value_scale"]), float(state["entropy_coef"])
        for k, v in counts.items():
            setattr(self, k, v)
