"""g2048_policy_encoder_mean (the "mean" reduction of the fused rollout encoder): exported, bound, and its argument checks
run before any device work.  CPU only."""
import ctypes as C


def test_mean_encoder_symbol_is_exported_and_bound():
    from src.g2048 import native as nv

    assert hasattr(C.CDLL(nv.LIB_PATH), "g2048_policy_encoder_mean")
    assert "g2048_policy_encoder_mean" in nv.SIGNATURES
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_mean_encoder_rejects_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": must be rejected before any use
    assert lib.g2048_policy_encoder_mean(None, None, None, None, None, 4, None, 8, None) == -1
    assert lib.g2048_policy_encoder_mean(None, a, a, a, a, 4, a, 8, None) == -1           # no boards
    assert lib.g2048_policy_encoder_mean(a, a, a, a, a, 4, None, 8, None) == -1           # no features
    assert lib.g2048_policy_encoder_mean(a, a, a, a, a, 0, a, 8, None) == -1              # no layers
    assert lib.g2048_policy_encoder_mean(a, a, a, a, a, 4, a, 0, None) == -1              # B = 0
    assert lib.g2048_policy_encoder_mean(a, a, a, a, a, 4, a, -3, None) == -1             # B < 0
    assert lib.g2048_policy_encoder_mean(a, a, a, a + 2, a, 4, a, 8, None) == -1          # weights not 16-byte aligned
    assert lib.g2048_policy_encoder_mean(a, a, a, a, a + 4, 4, a, 8, None) == -1          # params not 16-byte aligned
    assert lib.g2048_policy_encoder_mean(a, a + 8, a, a, a, 4, a, 8, None) == -1          # embed table not 16-byte aligned
    assert lib.g2048_policy_encoder_mean(a, a, a + 4, a, a, 4, a, 8, None) == -1          # CLS token not 16-byte aligned
    assert lib.g2048_policy_encoder_mean(a, a, a, a, a, 4, a + 4, 8, None) == -1          # features not 16-byte aligned


def test_mean_agent_selection_without_a_device():
    """A CPU agent never selects the fused encoder; supports() keeps meaning "cls" only."""
    from src.ppo import PPOAgent
    from src.ppo.fused_policy import supports, supports_mean

    mean_agent = PPOAgent(reduction="mean")
    assert not supports_mean(mean_agent)  # parameters on the CPU
    assert not supports(mean_agent)
    assert not supports_mean(PPOAgent(reduction="cls"))
