"""Imitation loss (g2048_distill_*): declared, bound, exported; every argument check runs before any device work; the wrappers refuse
host tensors and DistillTrainer bad settings without a device; the float64 restatement (tests/distill_ref.py) has the gradients
torch.autograd gives the same loss, its planted rows keep their promises and its inputs leave no sample undecided; the per-sample code of
the kernels, compiled for the host, stays within the restatement's bounds.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import distill_ref as D  # noqa: E402
import ntuple_ref as N  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_distill_loss": 19, "g2048_distill_loss_workspace_floats": 1, "g2048_distill_gather": 12}


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    assert "imitation update: loss" in header
    for name, nargs in NAMES.items():
        assert f" {name}(" in header
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert hasattr(lib, name)
        assert callable(getattr(nv, name[len("g2048_"):]))
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_workspace_size():
    from src.g2048 import native as nv

    lib = nv.load()
    cap = nv.CONSTANTS["G2048_PPO_LOSS_MAX_BATCH"]
    assert [lib.g2048_distill_loss_workspace_floats(m) for m in (1, 256, 257, 2055, cap)] == [5, 5, 10, 45, 5 * cap // 256]
    assert [lib.g2048_distill_loss_workspace_floats(m) for m in (0, -4, cap + 1)] == [-1, -1, -1]
    with pytest.raises(nv.NativeError):
        nv.distill_loss_workspace_floats(0)


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    cap = nv.CONSTANTS["G2048_PPO_LOSS_MAX_BATCH"]

    def loss(logits=a, lbf=0, values=a, vbf=0, mask=a, q=a, vt=a, M=8, tau=0.0, new_logp=a, sums=a, dlogits=a, dvalues=a, scale=a,
             running=a, ws=a):
        return lib.g2048_distill_loss(logits, lbf, values, vbf, mask, q, vt, M, tau, 0.5, 0.01, new_logp, sums, dlogits, dvalues, scale,
                                      running, ws, None)

    bad = [dict(logits=None), dict(q=None), dict(new_logp=None), dict(sums=None), dict(dlogits=None), dict(ws=None),
           # values, value_target and dvalues are given together or not at all
           dict(values=None), dict(vt=None), dict(dvalues=None), dict(values=None, vt=None), dict(values=None, dvalues=None),
           dict(vt=None, dvalues=None),
           dict(M=0), dict(M=-3), dict(M=cap + 1),
           dict(tau=-1.0), dict(tau=-1e-30), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau=float("-inf")),
           dict(q=a + 4), dict(q=a + 8), dict(logits=a + 2), dict(dlogits=a + 2), dict(logits=a + 1, lbf=1), dict(dlogits=a + 1, lbf=1),
           dict(values=a + 2), dict(dvalues=a + 2), dict(values=a + 1, vbf=1), dict(dvalues=a + 1, vbf=1), dict(vt=a + 2),
           dict(new_logp=a + 2), dict(sums=a + 1), dict(scale=a + 2), dict(running=a + 4), dict(ws=a + 2)]
    for kw in bad:
        assert loss(**kw) == -1, kw

    def gather(idx=a, M=8, n=100, boards=a, masks=a, q=a, vt=a, o_boards=a, o_masks=a, o_q=a, o_vt=a):
        return lib.g2048_distill_gather(idx, M, n, boards, masks, q, vt, o_boards, o_masks, o_q, o_vt, None)

    for kw in [dict(idx=None), dict(boards=None), dict(masks=None), dict(q=None), dict(o_boards=None), dict(o_masks=None), dict(o_q=None),
               dict(vt=None), dict(o_vt=None), dict(M=0), dict(M=-1), dict(n=0), dict(boards=a + 8), dict(o_boards=a + 4), dict(q=a + 8),
               dict(o_q=a + 4), dict(idx=a + 4), dict(vt=a + 2), dict(o_vt=a + 1)]:
        assert gather(**kw) == -1, kw


def test_wrappers_refuse_host_tensors():
    from src.g2048 import native as nv

    M = 4
    logits, v, q = torch.zeros(M, 4), torch.zeros(M), torch.zeros(M, 4)
    mask = torch.full((M,), 15, dtype=torch.uint8)
    with pytest.raises(nv.NativeError):
        nv.distill_loss(logits, v, mask, q, v.clone(), 0.0, 0.5, 0.01)
    with pytest.raises(nv.NativeError):
        nv.distill_loss(logits, None, None, q, None, 1.0, 0.0, 0.0)
    with pytest.raises(nv.NativeError):
        nv.distill_loss(logits, v, mask, q, None, 0.0, 0.5, 0.01)  # values without value_target
    boards = torch.zeros((10, 16), dtype=torch.uint8)
    with pytest.raises(nv.NativeError):
        nv.distill_gather(torch.zeros(M, dtype=torch.int64), boards, torch.zeros(10, dtype=torch.uint8), torch.zeros(10, 4), torch.zeros(10))
    with pytest.raises(nv.NativeError):
        nv.distill_gather(torch.zeros(M, dtype=torch.int64), boards, torch.zeros(10, dtype=torch.uint8), torch.zeros(10, 4))


def _small_agent():
    from src.ppo import PPOAgent

    return PPOAgent(observation_dim=31, action_dim=4, hidden_dim=32, d_model=32, nhead=2, num_layers=1, dim_feedforward=32, dropout=0.0,
                    reduction="cls")


def test_trainer_settings_and_state_without_a_device():
    from src.ppo import DistillTrainer, NTupleActionFunction, NTupleNetwork, PPOAgent

    net = NTupleNetwork(N.SMALL, device="cpu")
    agent = _small_agent()
    ok = dict(num_envs=64, capacity=512, batch_size=128, device="cpu")
    for bad in (dict(beta=-0.01), dict(beta=1.01), dict(beta=float("nan")), dict(tau=-0.5), dict(tau=float("inf")), dict(tau=float("nan")),
                dict(capacity=127), dict(num_envs=0), dict(num_envs=-2), dict(value_coef=-1.0), dict(value_coef=float("nan")),
                dict(value_coef=float("inf"))):
        with pytest.raises(ValueError):
            DistillTrainer(agent, net, **dict(ok, **bad))
    with pytest.raises(ValueError):
        DistillTrainer(PPOAgent(observation_dim=31, action_dim=3, hidden_dim=32, d_model=32, nhead=2, num_layers=1, dim_feedforward=32),
                       net, **ok)
    with pytest.raises(ValueError):
        DistillTrainer(agent, object(), **ok)  # no policy_fn
    tr = DistillTrainer(agent, net, value_coef=0.0, **ok)  # zero is allowed
    assert isinstance(tr.teacher, NTupleActionFunction) and tr.teacher.plies == 0 and tr.teacher.network is net
    assert tr.n_teacher == 32 and tr.ring["boards"].shape == (512, 16) and tr.ring["q"].shape == (512, 4)
    assert DistillTrainer(agent, NTupleActionFunction(net, plies=2), beta=1.0, **ok).n_teacher == 64
    assert DistillTrainer(agent, net, beta=0.0, **ok).n_teacher == 0
    assert DistillTrainer(agent, net, beta=0.7, num_envs=10, capacity=512, batch_size=128, device="cpu").n_teacher == 7
    assert DistillTrainer(agent, net, beta=0.01, **ok).n_teacher == 1  # ceil
    with pytest.raises(ValueError):
        tr.update(1)  # nothing collected yet
    tr.lock_steps, tr.updates, tr.rows = 5, 7, 320
    state = tr.state_dict()
    assert state["tau"] == 0.0 and state["beta"] == 0.5 and (state["lock_steps"], state["updates"], state["rows"]) == (5, 7, 320)
    fresh = DistillTrainer(agent, net, tau=2.0, beta=1.0, value_coef=0.25, **ok)
    fresh.load_state_dict(state)
    assert fresh.state_dict() == state and fresh.n_teacher == 32
    with pytest.raises(ValueError):
        DistillTrainer(agent, net, num_envs=32, capacity=512, batch_size=128, device="cpu").load_state_dict(state)
    with pytest.raises(ValueError):
        fresh.load_state_dict(dict(state, beta=3.0))
    with pytest.raises(ValueError):
        fresh.load_state_dict({k: v for k, v in state.items() if k != "updates"})
    assert fresh.state_dict() == state  # a refused state changes nothing


# ---------------------------------------------------------------------------------------------- the restatement
def _cases():
    for M in (63, 257):
        for masks in (True, False):
            for tau in D.TAUS:
                yield M, masks, tau


@pytest.mark.parametrize("M,masks,tau", list(_cases()))
def test_reference_gradients_equal_autograd(M, masks, tau):
    d = D.inputs(M, masks=masks)
    ref = D.distill_ref(d["logits"], d["values"], d["mask_bits"], d["teacher_q"], d["value_target"], tau, D.C_VALUE, D.C_ENTROPY)
    D.planted_expectations(ref, d, tau)
    lg = d["logits"].double().requires_grad_(True)
    vv = d["values"].double().requires_grad_(True)
    loss = D.torch_loss64(lg, vv, d["mask_bits"], d["teacher_q"], d["value_target"], tau, float(np.float32(D.C_VALUE)),
                          float(np.float32(D.C_ENTROPY)))
    loss.backward()
    inv_m = float(np.float32(1.0) / np.float32(M))  # the reference scales by the kernel's f32(1 / M)
    torch.testing.assert_close(ref["dlogits"].v, lg.grad * (inv_m * M), rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(ref["dvalues"].v, vv.grad * (inv_m * M), rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(ref["terms"].v[:, 3].sum() / M, loss.detach(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("M", D.MS)
def test_generated_inputs_leave_no_sample_undecided(M):
    for bf16 in (False, True):
        for masks in (True, False):
            d = D.inputs(M, bf16=bf16, masks=masks)
            ref = D.distill_ref(d["logits"], d["values"], d["mask_bits"], d["teacher_q"], d["value_target"], 1.0, D.C_VALUE, D.C_ENTROPY)
            assert D.undecided_share(ref, D.N_PLANTED) == 0.0 and not ref["undecided"].any()
            legal = ref["legal"][D.N_PLANTED:]
            z = D.masked32(d["logits"].float()[D.N_PLANTED:], legal)
            q = D.masked32(d["teacher_q"][D.N_PLANTED:], legal)
            if z.numel():
                assert float(D.top_gap(z).min()) >= 1e-3 and float(D.top_gap(q).min()) >= 1e-3


# ---------------------------------------------------------------------------------------------- the kernels' per-sample code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "distill_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libdistill_host.so")
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-o", so, HOST_SRC])
    return C.CDLL(so)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def host_loss(host, d, tau, scale=None):
    M = d["teacher_q"].shape[0]
    logits, values = d["logits"].contiguous(), d["values"]
    new_logp, sums = torch.full((M,), -7.0), torch.full((5,), -7.0)
    dlogits = torch.full_like(logits, -7.0)
    dvalues = None if values is None else torch.full_like(values, -7.0)
    running = torch.ones(5, dtype=torch.float64)
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32)
    host.hst_distill_loss(_p(logits), C.c_int(int(logits.dtype == torch.bfloat16)), _p(values),
                          C.c_int(int(values is not None and values.dtype == torch.bfloat16)), _p(d["mask_bits"]), _p(d["teacher_q"]),
                          _p(d["value_target"]), C.c_int64(M), C.c_float(tau), C.c_float(D.C_VALUE), C.c_float(D.C_ENTROPY), _p(new_logp),
                          _p(sums), _p(dlogits), _p(dvalues), _p(sc), _p(running))
    assert torch.equal(running, 1.0 + sums.double())
    return new_logp, sums, dlogits, dvalues


@pytest.mark.parametrize("M", D.MS)
@pytest.mark.parametrize("bf16", [False, True])
def test_host_build_stays_within_the_bounds(host, M, bf16):
    for masks in (True, False):
        for with_v in (True, False):
            for tau, scale in zip(D.TAUS, D.SCALES):
                d = D.inputs(M, bf16=bf16, masks=masks, values=with_v)
                ref = D.distill_ref(d["logits"], d["values"], d["mask_bits"], d["teacher_q"], d["value_target"], tau, D.C_VALUE,
                                    D.C_ENTROPY, scale)
                D.planted_expectations(ref, d, tau)
                got = host_loss(host, d, tau, scale)
                bad = D.distill_check(ref, *got, planted=D.N_PLANTED, show=f"host M={M} bf16={bf16} masks={masks} v={with_v} tau={tau}")
                assert not bad, bad
                assert float(got[1][4]) == float(np.float32(np.float32(ref["terms"].v[:, 4].sum()) * (np.float32(1) / np.float32(M))))
                if not with_v:
                    assert float(got[1][1]) == 0.0


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-sample code as a stand-alone program under ASan + UBSan over the planted rows: an access outside an array aborts it."""
    exe = str(tmp_path / "distill_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DDISTILL_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "distill_host ok" in out.stdout, (out.returncode, out.stderr[-2000:])
