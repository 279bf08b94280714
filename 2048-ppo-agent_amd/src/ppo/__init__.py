from .data_loader import create_ppo_dataloader
from .distill import DistillTrainer
from .expectimax import ExpectimaxActionFunction
from .lookahead import LookaheadActionFunction
from .monte_carlo import MonteCarloActionFunction
from .ntuple import (DEFAULT_TUPLES, NTupleActionFunction, NTupleBudgetSearchActionFunction, NTupleNetwork, NTupleSearchActionFunction,
                     NTupleTrainer)
from .ppo_agent import MLPAgent, PPOAgent
from .ppo_trainer import PPOTrainer
from .rollout_buffer import RolloutBuffer
from .torch_action_wrapper import TorchActionFunction, resolve_symmetry
