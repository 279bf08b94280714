"""The LAMB entry points (g2048_lamb_step / g2048_lamb_workspace_floats): declared, bound, exported, their argument checks run
before any device work; FlatLambStep.supports refuses what the kernels cannot run.  CPU only."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("g2048_lamb_step", "g2048_lamb_workspace_floats")
EINVAL = -1


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    assert "int g2048_lamb_step(" in header and "int64_t g2048_lamb_workspace_floats(" in header
    assert "} g2048_lamb_group;" in header and "lamb.py:106-209" in header
    for name in NAMES:
        assert name in nv.SIGNATURES
        assert hasattr(lib, name)
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays
    for fn in ("lamb_step", "lamb_workspace"):
        assert callable(getattr(nv, fn))
    # g2048_lamb_group: six doubles and four int32, no padding
    assert C.sizeof(nv.LambGroup) == 6 * 8 + 4 * 4
    assert [f[0] for f in nv.LambGroup._fields_] == ["lr", "beta1", "beta2", "beta3", "eps", "weight_decay", "bias_correction",
                                                     "adapt", "trust_clip", "reserved"]


def test_workspace_size():
    from src.g2048 import native as nv

    lib = nv.load()
    assert lib.g2048_lamb_workspace_floats(0) == 0 and lib.g2048_lamb_workspace_floats(-3) == 0
    # three partials per chunk (each list padded to a multiple of four floats), four flags, twelve floats per group
    assert lib.g2048_lamb_workspace_floats(1) == 3 * 4 + 4 + nv.OPT_MAX_GROUPS * 12
    assert lib.g2048_lamb_workspace_floats(1941) == 3 * 1944 + 4 + nv.OPT_MAX_GROUPS * 12
    assert lib.g2048_lamb_workspace_floats(1941) > lib.g2048_opt_workspace_floats(1941)


def test_entry_point_rejects_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": must be rejected before any use
    groups = (nv.LambGroup * 5)(*[nv.LambGroup(1e-3, 0.9, 0.999, 0.1, 1e-6, 0.01, 1, 0, 0, 0)] * 5)
    g = C.cast(groups, C.c_void_p)

    def call(chunks=a, n_chunks=3, grads=a, m=a, v=a, grp=g, n_groups=2, steps=a, n_steps=1, scale=None, tracker=None, ws=a):
        return lib.g2048_lamb_step(chunks, n_chunks, grads, m, v, grp, n_groups, 0.5, 1.0, steps, n_steps, scale, tracker, 2.0, 0.5,
                                   2000, ws, None, None)

    assert call(chunks=None) == EINVAL
    assert call(grads=None) == EINVAL
    assert call(m=None) == EINVAL
    assert call(v=None) == EINVAL
    assert call(grp=None) == EINVAL
    assert call(steps=None) == EINVAL
    assert call(ws=None) == EINVAL
    assert call(n_chunks=0) == EINVAL and call(n_chunks=-1) == EINVAL
    assert call(n_groups=0) == EINVAL
    assert call(n_groups=nv.OPT_MAX_GROUPS + 1) == EINVAL  # too many groups
    assert call(n_steps=0) == EINVAL
    assert call(grads=a + 4) == EINVAL and call(m=a + 8) == EINVAL and call(v=a + 4) == EINVAL and call(ws=a + 4) == EINVAL
    assert call(scale=a, tracker=None) == EINVAL  # a scale without a growth tracker


def test_wrappers_refuse_host_tensors_and_too_many_groups():
    from src.g2048 import native as nv

    z = torch.zeros(16)
    grp = (1e-3, 0.9, 0.999, 0.1, 1e-6, 0.01, True, False, False)
    with pytest.raises(nv.NativeError):
        nv.lamb_step(torch.zeros(64, dtype=torch.uint8), 1, z, z, z, [grp], 0.5, 1.0, torch.zeros(1), None, None, 2.0, 0.5, 2000, z)
    with pytest.raises(nv.NativeError):
        nv.lamb_step(torch.zeros(64, dtype=torch.uint8), 1, z, z, z, [grp] * 5, 0.5, 1.0, torch.zeros(1), None, None, 2.0, 0.5, 2000, z)


def test_supports():
    from src.optim import Lamb
    from src.optim.flat_step import FlatAdamWStep, FlatLambStep, flat_step_for

    ps = [torch.nn.Parameter(torch.zeros(4, 4)) for _ in range(5)]
    assert not FlatLambStep.supports(torch.optim.AdamW(ps), "cuda")  # another optimiser
    assert not FlatLambStep.supports(Lamb(ps), "cpu")                # a CPU run keeps the PyTorch calls
    assert not FlatLambStep.supports(Lamb(ps), "cuda")               # ... and so do parameters that are not on the device
    assert not FlatLambStep.supports(Lamb([{"params": [p]} for p in ps]), "cuda")  # five groups
    assert not FlatAdamWStep.supports(Lamb(ps), "cuda")
    assert flat_step_for(Lamb(ps), "cpu") is None and flat_step_for(torch.optim.Adam(ps), "cpu") is None
    with pytest.raises(ValueError):
        FlatLambStep(Lamb(ps), "cpu")
    for name in ("supports", "adopt_state", "reset_state", "adopt_shadows", "step", "sync_step_counts"):
        assert callable(getattr(FlatLambStep, name)) and callable(getattr(FlatAdamWStep, name))
