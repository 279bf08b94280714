"""g2048_lamb_step (clip + LAMB + GradScaler in three launches, FlatLambStep) against the PyTorch calls of the reference's update
loop with ``opt_name: lamb`` (src/ppo/ppo_trainer.py:413-434 around src/optim/lamb.py:106-209).

The error bound of the arithmetic tests: three runs of the same steps -- ``Lamb`` in f64 (the truth), ``Lamb`` in f32 (the
yardstick), the flat step.  Per tensor, relative to the tensor's largest magnitude in the truth, the flat step's largest error may
be at most 2 x the yardstick's plus one f32 ulp of that magnitude (the two f32 runs differ in the order in which three norms are
summed, the same error class; 2 is a margin, not a measurement).  Set G2048_LAMB_RATIOS_OUT=<file> to get, per case, the largest
measured ratio and every tensor above 2 as JSON (profiles/lamb_flat_step.json holds one such run).  Ratios above 2 were measured on small tensors only (1 to 256 elements: a moment of b.bias 6.99, of b.weight 2.01, of a 64-element
LayerNorm weight 3.37 and of a 256-element head weight 2.38 in the trainer epoch): there the "largest error of the tensor" is the
largest of a few draws of a handful of roundings, the f32 yardstick's draw can be a small fraction of an ulp (0.17 ulp on b.bias
against 1.2 ulp of the flat step), and the quotient of two such draws says little.  All of them are below one ulp + 2 x the
yardstick, which is what the floor is for; no tensor of more than 256 elements was measured above 2."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.amp import GradScaler

from src.g2048 import native as nv
from src.optim import Lamb, configure_bert_optimizers
from src.optim.flat_step import FlatAdamWStep, FlatLambStep
from src.ppo import PPOAgent, PPOTrainer, RolloutBuffer
from src.runs import BatchRunner

pytestmark = pytest.mark.gpu
OPTIM = dict(opt_name="lamb", max_lr=4e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, warmup_steps_ratio=0.025,
             scheduler_names=["linear", "cosine"], blacklist_weight_modules=["norm", "embedding"])
REF = np.load(os.path.join(os.path.dirname(__file__), "golden", "torch_reference.npz"))
_RATIOS = {}


class _Net(nn.Module):
    """The shapes of tests/test_gpu_optim.py::_Net (> 1 chunk, ragged tails, a scalar, both decay groups, tensors of 1 to 8 chunks)
    plus one [1024][256] weight: 128 chunks, the longest list of per-tensor partials of the real agent."""

    def __init__(self, extra=False):
        super().__init__()
        self.a = nn.Linear(300, 41)
        self.norm = nn.LayerNorm(41)
        self.b = nn.Linear(41, 1)
        self.embedding = nn.Embedding(7, 3)
        self.big = nn.Parameter(torch.randn(5000, 3))
        self.wide = nn.Linear(256, 1024, bias=False)
        if extra:
            self.zeros = nn.Parameter(torch.zeros(2100))  # ||p|| = 0 in the first step: r = 1


def _record(case, name, ratio):
    _RATIOS.setdefault(case, {})[name] = ratio


def _flush():
    """Per case the largest ratio and every tensor above 2 (those pass through the one-ulp floor only), if a file is asked for."""
    out = os.environ.get("G2048_LAMB_RATIOS_OUT")
    if not out:
        return
    brief = {}
    for case, d in _RATIOS.items():
        known = {k: v for k, v in d.items() if v["ratio"] is not None}
        top = max(known, key=lambda k: known[k]["ratio"])
        brief[case] = {"tensors": len(d), "max_ratio": round(known[top]["ratio"], 3), "at": top,
                       "above_2": {k: {"ratio": round(v["ratio"], 3), "flat_err": v["flat_err"], "f32_err": v["f32_err"],
                                       "elements": v["elements"]} for k, v in known.items() if v["ratio"] > 2.0}}
    with open(out, "w") as fh:
        json.dump(brief, fh, indent=1, sort_keys=True)


def _check_bound(case, name, flat, f32, f64):
    """The bound of the module docstring for one tensor; prints and records flat error / yardstick error."""
    f64 = f64.double()
    mag = float(f64.abs().max())
    if mag == 0.0:
        assert not bool(flat.any()) and not bool(f32.any()), (case, name)
        return
    e_flat = float((flat.double() - f64).abs().max()) / mag
    e_f32 = float((f32.double() - f64).abs().max()) / mag
    ulp = float(np.spacing(np.float32(mag))) / mag
    ratio = e_flat / e_f32 if e_f32 > 0 else (0.0 if e_flat == 0 else float("inf"))
    print(f"{case} {name}: flat {e_flat:.3e} f32 {e_f32:.3e} ratio {ratio:.3f} ulp {ulp:.3e}")
    _record(case, name, {"flat_err": e_flat, "f32_err": e_f32, "ratio": ratio if np.isfinite(ratio) else None, "elements": flat.numel()})
    assert e_flat <= 2.0 * e_f32 + ulp, (case, name, e_flat, e_f32, ulp)


# the gradient recipe of test_flat_step_matches_torch_sequence (unit normal times 30 on odd steps, times a small factor on even
# ones); the small factor cycles so that the norms (about 540 x the factor) fall on both sides of every threshold in play: the
# trainer's 0.5 or 4.0 and LAMB's own 1.0 (0.005 -> 2.7: with the trainer's clip at 4.0 only LAMB's binds)
_SMALL = (0.01, 0.0005, 0.005, 0.001, 0.01)


def _three_runs(dev, case, max_norm, with_scaler, lamb_kw=None, extra=False, zero_grad=(), steps=10):
    """``steps`` optimiser steps three times: Lamb f64 (no scaler: the overflow steps are left out by hand, the scale is a power of
    two), Lamb f32 through the torch sequence, FlatLambStep.  -> dict of the three nets / optimisers / the flat step."""
    torch.manual_seed(3)
    net_t = _Net(extra).to(dev)
    net_f = copy.deepcopy(net_t)
    net_d = copy.deepcopy(net_t).double()

    def mk(net):
        o = configure_bert_optimizers(net, steps=50, **OPTIM)
        if lamb_kw:
            for k, v in lamb_kw.items():
                if k == "max_grad_norm":
                    o["optimizer"].defaults[k] = v
                for grp in o["optimizer"].param_groups:
                    grp[k] = v
        return o

    ot, of, od = mk(net_t), mk(net_f), mk(net_d)
    assert type(of["optimizer"]) is Lamb
    st = GradScaler(init_scale=1024.0, growth_interval=3) if with_scaler else None
    sf = GradScaler(init_scale=1024.0, growth_interval=3) if with_scaler else None
    flat = FlatLambStep(of["optimizer"], dev)
    opt_t, opt_d = ot["optimizer"], od["optimizer"]
    names = [n for n, _ in net_t.named_parameters()]
    g = torch.Generator(device="cpu").manual_seed(11)
    infos = []
    for it in range(steps):
        scale = float(st.get_scale()) if with_scaler else 1.0
        big = 30.0 if it % 2 else _SMALL[(it // 2) % len(_SMALL)]
        grads = [torch.randn(p.shape, generator=g).to(dev) * big for p in net_t.parameters()]
        for i, n in enumerate(names):
            if n in zero_grad:
                grads[i].zero_()
        overflow = with_scaler and it in (4, 5)
        clean = [gr.clone() for gr in grads]
        if overflow:  # two consecutive overflow steps: skipped, scale halves twice
            grads[2][0] = float("inf") if it == 4 else float("nan")
        by_param = {id(q): gr for q, gr in zip(net_f.parameters(), grads)}
        for p, gr in zip(net_t.parameters(), grads):
            p.grad = gr * scale
        for v, q in zip(flat.grad_views, flat.params):  # the flat layout is ordered by parameter group
            v.copy_(by_param[id(q)] * scale)
        if with_scaler:
            st.scale(torch.zeros(1, device=dev))  # lazy init of the scale, as scaler.scale(loss) does in the loop
            st.unscale_(opt_t)
            torch.nn.utils.clip_grad_norm_(net_t.parameters(), max_norm)
            st.step(opt_t)
            st.update()
        else:
            torch.nn.utils.clip_grad_norm_(net_t.parameters(), max_norm)
            opt_t.step()
        if not overflow:
            for p, gr in zip(net_d.parameters(), clean):
                p.grad = gr.double()
            torch.nn.utils.clip_grad_norm_(net_d.parameters(), max_norm)
            opt_d.step()
        flat.step(max_norm, sf)
        for o in (ot, of, od):
            o["lr_scheduler"]["scheduler"].step()
        infos.append(flat.info.clone())
        if with_scaler:
            assert float(st.get_scale()) == float(sf.get_scale()), it
            assert int(st._growth_tracker.item()) == int(sf._growth_tracker.item()), it
            assert bool(flat.info[1].item()) == overflow, it
        else:
            assert float(flat.info[1]) == 0.0
        if not overflow:
            want = float(torch.linalg.vector_norm(torch.stack([c.double().norm() for c in clean])))
            assert abs(float(flat.info[0]) - want) <= 1e-5 * want, (it, float(flat.info[0]), want)
    for (n, p), q, d in zip(net_t.named_parameters(), net_f.parameters(), net_d.parameters()):
        _check_bound(case, n, q.detach(), p.detach(), d.detach())
        a, b, c = opt_t.state[p], of["optimizer"].state[q], opt_d.state[d]
        _check_bound(case, n + ":exp_avg", b["exp_avg"], a["exp_avg"], c["exp_avg"])
        _check_bound(case, n + ":exp_avg_sq", b["exp_avg_sq"], a["exp_avg_sq"], c["exp_avg_sq"])
    _flush()
    done = steps - 2 if with_scaler and steps > 5 else steps
    assert flat.sync_step_counts() == done
    assert all(grp["step"] == done for grp in opt_t.param_groups) and all(grp["step"] == done for grp in of["optimizer"].param_groups)
    return dict(net_t=net_t, net_f=net_f, net_d=net_d, flat=flat, opt_f=of["optimizer"], opt_t=opt_t, sf=sf, infos=infos)


def test_reference_fixtures(dev):
    """lamb/* of torch_reference.npz (written by the reference's Lamb) through FlatLambStep: two steps, no scaler, trainer clip off."""
    w = nn.Parameter(torch.from_numpy(REF["lamb/w0"].copy()).to(dev))
    b = nn.Parameter(torch.from_numpy(REF["lamb/b0"].copy()).to(dev))
    opt = Lamb([{"params": [w], "weight_decay": 0.01}, {"params": [b], "weight_decay": 0.0}], lr=1e-2)
    flat = FlatLambStep(opt, dev)
    for gw, gb in zip(REF["lamb/gw"], REF["lamb/gb"]):
        flat.grad_views[0].copy_(torch.from_numpy(gw.copy()))
        flat.grad_views[1].copy_(torch.from_numpy(gb.copy()))
        flat.step(0.0, None)
    np.testing.assert_allclose(w.detach().cpu().numpy(), REF["lamb/w2"], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(b.detach().cpu().numpy(), REF["lamb/b2"], atol=1e-6, rtol=1e-5)
    assert flat.sync_step_counts() == len(REF["lamb/gw"]) == 2


@pytest.mark.parametrize("max_norm", [0.5, 4.0])
@pytest.mark.parametrize("with_scaler", [True, False])
def test_flat_step_matches_torch_sequence(dev, with_scaler, max_norm):
    r = _three_runs(dev, f"sequence[scaler={int(with_scaler)},clip={max_norm}]", max_norm, with_scaler)
    if with_scaler:
        assert float(r["sf"].get_scale()) == 1024.0 * 2 / 4 * 2  # grew after 3 clean steps, halved twice, grew again


@pytest.mark.parametrize("kw", [dict(always_adapt=True), dict(trust_clip=True), dict(grad_averaging=False), dict(bias_correction=False),
                                dict(max_grad_norm=None), dict(always_adapt=True, trust_clip=True)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_options(dev, kw):
    """Each of Lamb's switches under the same bound; a tensor of zeros (||p|| = 0: r = 1, it moves by lr * u) and no-decay tensors
    whose gradient is always zero, so that u = 0: norm.bias (zeros: ||p|| = 0 as well) and norm.weight (ones: only ||u|| = 0
    selects r = 1 there; with always_adapt a kernel that tested ||p|| > 0 alone would form inf * 0).  Both stay bit for bit."""
    r = _three_runs(dev, "options[" + ",".join(f"{k}={v}" for k, v in kw.items()) + "]", 0.5, False, lamb_kw=kw, extra=True,
                    zero_grad=("norm.bias", "norm.weight"), steps=6)
    assert bool(r["net_f"].zeros.detach().abs().sum() > 0)
    assert torch.equal(r["net_f"].norm.bias.detach(), torch.zeros(41, device=dev))  # LayerNorm's bias starts at 0 and never moves
    assert torch.equal(r["net_f"].norm.weight.detach(), torch.ones(41, device=dev))  # ||p|| > 0, ||u|| = 0: r = 1, not inf
    assert torch.equal(r["net_f"].norm.bias.detach(), r["net_t"].norm.bias.detach())
    assert torch.equal(r["net_f"].norm.weight.detach(), r["net_t"].norm.weight.detach())
    assert all(bool(torch.isfinite(p).all()) for p in r["net_f"].parameters())


def test_first_step_from_zero_weights_uses_ratio_one(dev):
    """||p|| = 0 -> r = 1 exactly: one step on a tensor of zeros equals Lamb's, which then is p = -lr * u."""
    p, q = nn.Parameter(torch.zeros(3000, device=dev)), nn.Parameter(torch.zeros(3000, device=dev))
    opt, ref = Lamb([p], lr=1e-2, weight_decay=0.01), Lamb([q], lr=1e-2, weight_decay=0.01)
    flat = FlatLambStep(opt, dev)
    gr = torch.randn(3000, device=dev) * 1e-3  # norm 0.055: no clip binds
    flat.grad_views[0].copy_(gr)
    q.grad = gr.clone()
    ref.step()
    flat.step(0.0, None)
    torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-9)
    assert float(p.detach().abs().max()) > 1e-3  # moved by about lr, not by lr * ||p|| / ||u|| = 0


def test_skip_leaves_parameters_without_gradient_alone(dev):
    """A parameter in ``skip`` keeps parameter and moments bit for bit and is out of the norm: what Lamb does with p.grad None."""
    torch.manual_seed(2)
    ps = [nn.Parameter(torch.randn(300, 256, device=dev)), nn.Parameter(torch.randn(77, device=dev)),
          nn.Parameter(torch.randn(64, 32, device=dev))]
    ref = [nn.Parameter(p.detach().clone()) for p in ps]
    before = ps[1].detach().clone()
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.1)
    opt, opt_ref = Lamb(ps, **kw), Lamb(ref, **kw)
    fs = FlatLambStep(opt, dev)
    for step in range(3):
        g0, g2 = torch.randn_like(ps[0]), torch.randn_like(ps[2])
        fs.grad_views[0].copy_(g0)
        fs.grad_views[1].fill_(float("nan"))  # never read: the parameter is skipped
        fs.grad_views[2].copy_(g2)
        ref[0].grad, ref[1].grad, ref[2].grad = g0.clone(), None, g2.clone()
        torch.nn.utils.clip_grad_norm_([ref[0], ref[2]], 0.5)
        opt_ref.step()
        fs.step(0.5, None, skip=(1,))
        assert float(fs.info[1]) == 0.0 and bool(torch.isfinite(fs.info[0]))  # the NaN slice did not reach the norm
    np.testing.assert_allclose(ps[0].detach().cpu().numpy(), ref[0].detach().cpu().numpy(), atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(ps[2].detach().cpu().numpy(), ref[2].detach().cpu().numpy(), atol=1e-6, rtol=1e-5)
    assert torch.equal(ps[1].detach(), before) and torch.equal(ps[1].detach(), ref[1].detach())
    assert not bool(fs.m_views[1].any()) and not bool(fs.v_views[1].any())


def test_determinism(dev):
    """The same ten steps twice from the same state: parameters, moments and info bitwise equal."""
    a = _three_runs(dev, "determinism", 0.5, True)
    b = _three_runs(dev, "determinism", 0.5, True)
    for p, q in zip(a["net_f"].parameters(), b["net_f"].parameters()):
        assert torch.equal(p, q)
    assert torch.equal(a["flat"].exp_avg, b["flat"].exp_avg) and torch.equal(a["flat"].exp_avg_sq, b["flat"].exp_avg_sq)
    for x, y in zip(a["infos"], b["infos"]):
        assert torch.equal(x, y) or (bool(torch.isnan(x[0])) and bool(torch.isnan(y[0])) and x[1] == y[1])


def test_state_dict_round_trip(dev):
    """optimizer.state_dict() of the flat step (after sync_step_counts) loads into a plain Lamb and back."""
    torch.manual_seed(4)
    net_f = _Net().to(dev)
    net_t = copy.deepcopy(net_f)
    of, ot = configure_bert_optimizers(net_f, steps=50, **OPTIM), configure_bert_optimizers(net_t, steps=50, **OPTIM)
    flat = FlatLambStep(of["optimizer"], dev)
    for _ in range(2):
        for v in flat.grad_views:
            v.normal_()
        flat.step(0.5, None)
    assert flat.sync_step_counts() == 2
    sd = copy.deepcopy(of["optimizer"].state_dict())
    assert all(g["step"] == 2 for g in sd["param_groups"])
    ot["optimizer"].load_state_dict(sd)
    assert all(g["step"] == 2 for g in ot["optimizer"].param_groups)
    for p, q in zip(net_t.parameters(), net_f.parameters()):
        assert torch.equal(ot["optimizer"].state[p]["exp_avg"], of["optimizer"].state[q]["exp_avg"])
    net_n = copy.deepcopy(net_f)
    on = configure_bert_optimizers(net_n, steps=50, **OPTIM)
    flat_n = FlatLambStep(on["optimizer"], dev)
    on["optimizer"].load_state_dict(sd)
    flat_n.adopt_state()
    assert torch.equal(flat_n.exp_avg, flat.exp_avg) and torch.equal(flat_n.exp_avg_sq, flat.exp_avg_sq)
    assert float(flat_n.steps[0]) == 2.0
    for v, w in zip(flat.grad_views, flat_n.grad_views):
        w.copy_(v)
    flat.step(0.5, None)
    flat_n.step(0.5, None)
    for p, q in zip(net_f.parameters(), net_n.parameters()):
        assert torch.equal(p, q)
    # groups that disagree on the step count cannot be continued by one device count
    on["optimizer"].param_groups[0]["step"] = 7
    with pytest.raises(ValueError):
        flat_n.adopt_state()


def _trainer(dev, agent, log_dir, **kw):
    optim = dict(OPTIM, scheduler_names=["constant", "constant"])
    args = dict(gamma=0.99, lambda_gae=0.95, clip_epsilon=0.2, value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5,
                target_kl=10.0, use_action_mask=True, device=dev, mixed_precision="bfloat16", max_samples_per_epoch=1024,
                shuffle_on_reset=False, log_dir=str(log_dir))
    args.update(kw)
    return PPOTrainer(agent, BatchRunner(init_seed=0), RolloutBuffer(31, 16, 4), optim, max_steps=1000, **args)


def test_optimiser_keeps_bf16_shadows_current(dev, tmp_path, monkeypatch):
    """As tests/test_gpu_optim.py::test_optimiser_keeps_bf16_shadows_current, with LAMB: the shadows (dense, transposed, packed,
    packed-transposed) are maintained by k_lamb_apply, not by cast kernels in the graph, and equal a fresh cast bit for bit."""
    from src.ppo.hip_ops import Bf16Shadow

    monkeypatch.chdir(tmp_path)
    torch.manual_seed(11)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=2, dim_feedforward=1024, dropout=0.1, reduction="cls")
    tr = _trainer(dev, agent, tmp_path / "s", rollout_amp=True, max_samples_per_epoch=6 * 1024)
    assert type(tr._flat_step) is FlatLambStep and tr.use_hip_graph
    tr.collect_rollouts(batch_size=128, num_batches=1)
    before = [p.detach().clone() for p in agent.parameters()]
    m = tr.update_policy(batch_size=1024, n_epochs=1)
    assert m["hip_graph"] and m["n_updates"] >= 3
    assert all(not torch.equal(a, b) for a, b in zip(before, agent.parameters()) if a.numel() > 1)
    mine = {id(p) for p in agent.parameters()}
    shadows = [s for s in Bf16Shadow._live if s.views is not None and all(id(p) in mine for p in s.params)]
    assert len(shadows) >= 2 and all(s.maintainer is tr._flat_step for s in shadows)
    assert sum(len(s.packed) for s in shadows) == 7

    def check():
        for s in shadows:
            assert s.key == s.current_key()
            for i, (p, v) in enumerate(zip(s.params, s.views)):
                assert torch.equal(v, p.detach().to(torch.bfloat16)), i
            for i, tv in s.tviews.items():
                assert torch.equal(tv, s.params[i].detach().to(torch.bfloat16).t()), i
            for i in s.packed:
                ref = s.params[i].detach().to(torch.bfloat16)
                assert torch.equal(s.pviews[i], nv.pack_fragments(ref)) and torch.equal(s.ptviews[i], nv.pack_fragments(ref.t())), i

    check()
    tr.use_hip_graph = False  # an eager minibatch takes the same optimiser path
    tr.update_policy(batch_size=1024, n_epochs=1)
    check()


def test_trainer_epoch_under_the_three_run_bound(dev, tmp_path, monkeypatch):
    """One epoch of ``update_policy`` (dropout 0, several minibatches) under the flat step, held to the bound of this file: the
    gradient bucket of every minibatch is recorded as the step sees it and replayed, from the same initial parameters, into a plain
    ``Lamb`` in f32 (the PyTorch calls of G2048_FLAT_OPT=0: unscale, clip_grad_norm_, step) and in f64.  Replayed rather than
    taken from a second trainer, because only then do the three runs see the same gradients: a G2048_FLAT_OPT=0 trainer sums its
    gradients in another order (no flat bucket, no GradSink), and from the second minibatch on its forward runs on parameters that
    differ by rounding.  That pair of trainers is compared in the next test."""
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    agent = PPOAgent(hidden_dim=64, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, dropout=0.0, reduction="cls")
    tr = _trainer(dev, agent, tmp_path / "r", use_hip_graph=False)
    fs = tr._flat_step
    assert type(fs) is FlatLambStep
    names = {id(p): n for n, p in agent.named_parameters()}
    start = [p.detach().clone() for p in fs.params]

    def plain(dtype):
        ps = [nn.Parameter(p.to(dtype)) for p in start]
        by = {id(p): q for p, q in zip(fs.params, ps)}
        g0 = tr.optimizer.param_groups[0]
        groups = [{"params": [by[id(p)] for p in g["params"] if id(p) in by], "weight_decay": g["weight_decay"]}
                  for g in tr.optimizer.param_groups]
        return ps, Lamb(groups, lr=g0["lr"], betas=g0["betas"], eps=g0["eps"])

    (p32, o32), (p64, o64) = plain(torch.float32), plain(torch.float64)
    seen, inner = [], fs.step

    def recording_step(max_grad_norm, scaler=None, skip=()):
        assert not tuple(skip)
        scale = float(scaler.get_scale()) if scaler is not None and scaler.is_enabled() else 1.0
        seen.append((fs.grad.clone(), scale, max_grad_norm, [g["lr"] for g in tr.optimizer.param_groups]))
        inner(max_grad_norm, scaler, skip=skip)
        assert float(fs.info[1]) == 0.0  # no overflow: every recorded step was taken

    fs.step = recording_step
    tr.collect_rollouts(batch_size=64, num_batches=1)
    torch.manual_seed(6)
    m = tr.update_policy(batch_size=256, n_epochs=1)
    fs.step = inner
    assert m["n_updates"] == len(seen) >= 4
    for bucket, scale, max_norm, lrs in seen:
        for ps, opt, dt in ((p32, o32, torch.float32), (p64, o64, torch.float64)):
            for q, off, p in zip(ps, fs.offsets, fs.params):
                gr = bucket[off:off + p.numel()].view_as(p)
                q.grad = (gr * (1.0 / scale)).to(dt) if dt is torch.float32 else gr.double() / scale
            for g, lr in zip(opt.param_groups, lrs):
                g["lr"] = lr
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
    for p, a, b in zip(fs.params, p32, p64):
        _check_bound("trainer_epoch", names[id(p)], p.detach(), a.detach(), b.detach())
        _check_bound("trainer_epoch", names[id(p)] + ":exp_avg", tr.optimizer.state[p]["exp_avg"], o32.state[a]["exp_avg"], o64.state[b]["exp_avg"])
        _check_bound("trainer_epoch", names[id(p)] + ":exp_avg_sq", tr.optimizer.state[p]["exp_avg_sq"], o32.state[a]["exp_avg_sq"],
                     o64.state[b]["exp_avg_sq"])
    _flush()
    assert fs.sync_step_counts() == len(seen) == o32.param_groups[0]["step"]


def test_trainer_picks_the_lamb_step_and_matches_the_torch_calls(dev, tmp_path, monkeypatch):
    """opt_name "lamb": the trainer holds a FlatLambStep and replays the hipGraph on the default agent (4 layers, cls);
    G2048_FLAT_OPT=0 keeps the PyTorch calls.  The same rollouts and minibatches through both: after one step and after one epoch of
    several minibatches the displacements and the loss agree as tests/test_gpu_optim.py::
    test_trainer_update_with_flat_step_matches_torch_step asks of AdamW, with that test's bounds.  These two trainers do not see the
    same gradients (GradSink's summation order against at::sum's, then forwards on parameters that differ by rounding; LAMB's
    m / sqrt(v) turns an element whose gradient is near zero into +-lr either way), so the three-run bound is held by the replay of
    the test above, not here.  Then checkpoints both ways with the right step count."""
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(1)
    big = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024, dropout=0.0, reduction="cls")
    tr = _trainer(dev, big, tmp_path / "g", rollout_amp=True, max_samples_per_epoch=2048)
    assert type(tr._flat_step) is FlatLambStep
    tr.collect_rollouts(batch_size=64, num_batches=1)
    m = tr.update_policy(batch_size=1024, n_epochs=1)
    assert m["hip_graph"] is True and m["n_updates"] >= 1 and np.isfinite(m["total_loss"])

    def run(flat, batch, epochs):
        monkeypatch.setenv("G2048_FLAT_OPT", "1" if flat else "0")
        torch.manual_seed(5)
        agent = PPOAgent(hidden_dim=64, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, dropout=0.0, reduction="cls")
        t = _trainer(dev, agent, tmp_path / ("f" if flat else "t"), use_hip_graph=False)
        assert (type(t._flat_step) is FlatLambStep) == flat and (t._flat_step is not None) == flat
        t.collect_rollouts(batch_size=64, num_batches=1)
        torch.manual_seed(6)
        return t, t.update_policy(batch_size=batch, n_epochs=epochs)

    torch.manual_seed(5)
    init = PPOAgent(hidden_dim=64, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, dropout=0.0, reduction="cls")
    p0 = torch.cat([p.detach().flatten() for p in init.parameters()]).to(dev)
    disp = lambda t: torch.cat([p.detach().flatten() for p in t.agent.parameters()]) - p0
    (tr_f, m_f), (tr_t, m_t) = run(True, 1024, 1), run(False, 1024, 1)
    assert m_f["n_updates"] == m_t["n_updates"] == 1
    rel = float((disp(tr_f) - disp(tr_t)).norm() / disp(tr_t).norm())
    print("one step, relative difference of the displacements:", rel)
    assert rel < 2e-2
    tr_f, m_f = run(True, 256, 1)
    tr_t, m_t = run(False, 256, 1)
    n = m_f["n_updates"]
    assert n == m_t["n_updates"] >= 4
    df, dt = disp(tr_f), disp(tr_t)
    rel = float((df - dt).norm() / dt.norm())
    print(f"one epoch of {n} minibatches, relative difference of the displacements:", rel, "losses", m_f["total_loss"], m_t["total_loss"])
    assert float(df.norm()) > 0 and rel < 0.25
    np.testing.assert_allclose(m_f["total_loss"], m_t["total_loss"], rtol=2e-2, atol=1e-3)
    # checkpoint written under the flat step loads into the PyTorch-call trainer and the other way round
    tr_f.save_checkpoint(str(tmp_path / "f.pt"))
    assert all(g["step"] == n for g in tr_f.optimizer.param_groups)
    tr_t.load_checkpoint(str(tmp_path / "f.pt"), load_optimizer=True)
    assert all(g["step"] == n for g in tr_t.optimizer.param_groups)
    for p, q in zip(tr_f.agent.parameters(), tr_t.agent.parameters()):
        assert torch.equal(p, q) and torch.equal(tr_f.optimizer.state[p]["exp_avg_sq"], tr_t.optimizer.state[q]["exp_avg_sq"])
    # one more identical step on both sides (the same gradients, handed to both optimisers directly)
    gen = torch.Generator(device="cpu").manual_seed(1)
    fs = tr_f._flat_step
    for p, q, v in zip(fs.params, [dict(zip(map(id, tr_f.agent.parameters()), tr_t.agent.parameters()))[id(p)] for p in fs.params],
                       fs.grad_views):
        gr = (torch.randn(p.shape, generator=gen) * 1e-2).to(dev)
        v.copy_(gr)
        q.grad = gr.clone()
    torch.nn.utils.clip_grad_norm_(tr_t.agent.parameters(), 0.5)
    tr_t.optimizer.step()
    fs.step(0.5, None)
    assert fs.sync_step_counts() == n + 1 == tr_t.optimizer.param_groups[0]["step"]
    for p, q in zip(tr_f.agent.parameters(), tr_t.agent.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), atol=1e-6, rtol=1e-5)
    # and back
    tr_t.save_checkpoint(str(tmp_path / "t.pt"))
    tr_f.load_checkpoint(str(tmp_path / "t.pt"), load_optimizer=True)
    assert float(tr_f._flat_step.steps[0]) == n + 1
    m2 = tr_f.update_policy(batch_size=256, n_epochs=1)
    assert m2["n_updates"] >= 2 and np.isfinite(m2["total_loss"])
    assert tr_f._flat_step.sync_step_counts() == n + 1 + m2["n_updates"]


def test_adamw_still_gets_its_own_step(dev, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    agent = PPOAgent(hidden_dim=64, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, dropout=0.0, reduction="cls")
    tr = PPOTrainer(agent, BatchRunner(init_seed=0), RolloutBuffer(31, 16, 4), dict(OPTIM, opt_name="adamw", scheduler_names=["constant", "constant"]),
                    max_steps=100, device=dev, mixed_precision="bfloat16", log_dir=str(tmp_path / "a"))
    assert type(tr._flat_step) is FlatAdamWStep


def test_ppo_iteration_with_lamb(dev, tmp_path, monkeypatch):
    """A PPO iteration end to end with LAMB on a small board count: rollout and update policies agree (|kl| small)."""
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=2, dim_feedforward=1024, reduction="cls")
    tr = PPOTrainer(agent, BatchRunner(init_seed=0), RolloutBuffer(31, 16, 4), dict(OPTIM, scheduler_names=["constant", "constant"]),
                    max_steps=1000, gamma=0.99, lambda_gae=0.95, clip_epsilon=0.2, value_loss_coef=0.5, entropy_coef=0.01,
                    max_grad_norm=0.5, target_kl=0.25, use_action_mask=True, device=dev, mixed_precision="bfloat16",
                    max_samples_per_epoch=2000, shuffle_on_reset=True, rollout_amp=True)
    assert type(tr._flat_step) is FlatLambStep
    tr.collect_rollouts(64, 1)
    m = tr.update_policy(batch_size=256, n_epochs=1)
    assert m["n_updates"] >= 2 and np.isfinite(m["total_loss"]) and abs(m["kl_divergence"]) < 0.05
