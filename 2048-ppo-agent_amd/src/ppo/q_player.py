"""What a score-playing act_fn is: ``policy_fn(boards, masks) -> (q f32 [B, 4], v f32 [B])``, played by the engine's masked argmax.

The search players (one- and two-ply expectimax, Monte-Carlo playouts, the n-tuple network) differ in how they score a move, not in
how a score becomes a move: ``QPlayer`` is that common part.  It has no ``__init__`` and no state; a player mixes it in, sets
``self.rng_mode`` (anything ``resolve_rng_mode`` takes) and defines ``policy_fn``.
"""
import torch

from ..actions import _common as C


class QPlayer:
    use_mask = True  # the engine (``g2048_policy_step``) masks q by legality and takes the argmax: nothing is sampled
    sample_actions = False

    def _rng_mode(self) -> int:
        """``self.rng_mode`` as the kernels take it; an unknown spelling raises ``ValueError`` (``resolve_rng_mode``)."""
        return C.resolve_rng_mode(self.rng_mode)

    @staticmethod
    def best_legal(q: torch.Tensor, legal: torch.Tensor) -> torch.Tensor:
        """q f32 [B, 4], legal bool [B, 4] -> v f32 [B]: the max of q over the legal actions, +0 where there is none."""
        v = torch.where(legal, q, torch.full_like(q, float("-inf"))).max(dim=1).values
        return torch.where(legal.any(dim=1), v, torch.zeros_like(v))

    @torch.no_grad()
    def __call__(self, rng_key, obs, mask):
        """Un-batched plug-in protocol ``(rng_key[2], obs[4,4,31], mask[4]) -> (action, log_prob, value)``; leading batch
        dimensions are accepted (numpy arrays then, numpy scalars otherwise).  The one-hot observation is decoded to a packed
        board and goes down ``policy_fn``; the move is the masked argmax of ``q`` (``g2048_act_logits``)."""
        rows, batched = C.obs_rows(obs)
        q, values = self.policy_fn(rows.argmax(dim=-1).to(torch.uint8).to(C.device()), None)
        return C.act_on_logits(rng_key, q, values, mask, True, False, self._rng_mode(), batched)
