"""Golden composed configuration of the reference's Hydra tree (run where a checkout of the reference is present).

    python tests/golden/make_golden_configs.py <reference checkout>

Input  (never copied into this repo): <reference checkout>/configs/ -- train_ppo_agent.yaml and its groups
(data, model, trainer, paths, hydra, experiment), composed by this repository's own loader
(2048-ppo-agent_amd/run/config_tree.py) exactly as tests/test_host_logic.py composes a config tree.

Output (data only): tests/golden/reference_config_composed.json with two compositions:
  * "default": ``compose(train_ppo_agent.yaml)``
  * "resume":  ``compose(train_ppo_agent.yaml, ["+experiment=resume_train_ppo_agent", "trainer.rollout_batch_size=65536"])``
Values that depend on where and when the loader ran are made portable: a path under the working directory
starts with ``<work_dir>`` instead, and the ``hydra`` node (output directories stamped with the current time)
is reduced to its sorted keys.
"""
import importlib.util
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LOADER = os.path.join(HERE, "..", "..", "2048-ppo-agent_amd", "run", "config_tree.py")
OUT = os.path.join(HERE, "reference_config_composed.json")
RESUME = ["+experiment=resume_train_ppo_agent", "trainer.rollout_batch_size=65536"]


def _loader():
    spec = importlib.util.spec_from_file_location("config_tree", LOADER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _portable(node, cwd):
    if isinstance(node, dict):
        return {k: _portable(v, cwd) for k, v in node.items()}
    if isinstance(node, list):
        return [_portable(v, cwd) for v in node]
    if isinstance(node, str) and node.startswith(cwd):
        return "<work_dir>" + node[len(cwd):]
    return node


def composed(ct, configs, overrides=()):
    c = ct.compose(os.path.join(configs, "train_ppo_agent.yaml"), list(overrides))
    c = _portable(c, os.getcwd())
    c["hydra"] = sorted(c["hydra"])
    return c


if __name__ == "__main__":
    configs = os.path.join(os.path.abspath(sys.argv[1]), "configs")
    ct = _loader()
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as work:
        os.chdir(work)
        try:
            out = {"default": composed(ct, configs), "resume": composed(ct, configs, RESUME), "resume_overrides": RESUME}
        finally:
            os.chdir(here)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT)
