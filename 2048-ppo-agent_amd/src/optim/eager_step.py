"""The reference's optimiser step in PyTorch calls (what runs where no flat step does: flat_step.py) and the GradScaler's device
scale.  Both lean on private torch interfaces (src/ppo/torch_compat.py checks them); the trainers reach them only through here."""
import torch


def loss_scale(scaler, device):
    """The GradScaler's scale as the f32 [1] tensor it keeps on ``device`` (created here on first use), for kernels that apply the
    loss scale themselves; None without a scaler or with scaling off."""
    if scaler is None or not scaler.is_enabled():
        return None
    if scaler._scale is None:
        scaler._lazy_init_scale_growth_tracker(device)
    return scaler._scale


def eager_step(optimizer, scaler, parameters, max_grad_norm, device):
    """unscale -> global-norm clip -> step -> scale update (``scaler`` None: clip -> step) on gradients that are in place."""
    parameters = list(parameters)
    if scaler is not None:
        scaler.unscale_(optimizer)
        torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)
        scaler.step(optimizer)
        scaler.update()
    else:
        torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)
        optimizer.step()
    if device.type == "cuda":
        # torch's fused optimisers update the parameters without advancing autograd's version counters (measured: an eager
        # update kept running its forward on the bf16 shadows of the FIRST step); everything that caches derived weights keys
        # on them (Bf16Shadow, the fused rollout encoder's packed weights)
        torch.autograd.graph.increment_version(parameters)
