"""Which configurations the fused update path accepts, with and without RRL_FAST_BASELINES=1 (no GPU needed)."""
import pytest

import arg_utils
from recovery_rl_amd.fast_update import fast_path_supported


def cfg(*flags):
    return arg_utils.get_args(["--env-name", "navigation1"] + list(flags))


COMPARISON = {"LR": ["--DGD_constraints", "--nu", "5000", "--update_nu"],
              "RSPO": ["--DGD_constraints", "--nu_schedule", "--nu_start", "10000"],
              "SQRL": ["--DGD_constraints", "--use_constraint_sampling", "--nu", "5000", "--update_nu"],
              "RCPO": ["--RCPO", "--lambda_RCPO", "1000"],
              "update_nu": ["--update_nu"], "sampling": ["--use_constraint_sampling"], "schedule": ["--nu_schedule"]}
RECOVERY_RL = {"MF": ["--use_recovery", "--MF_recovery"], "MB": ["--use_recovery"], "unconstrained": [],
               "RP": ["--constraint_reward_penalty", "1000"]}
NEVER = {"autoent": ["--automatic_entropy_tuning", "True"], "deterministic": ["--policy", "Deterministic"],
         "interval": ["--target_update_interval", "2"]}


@pytest.mark.parametrize("switch", (None, "0", "1"))
def test_fast_path_supported_matrix(monkeypatch, switch):
    if switch is None:
        monkeypatch.delenv("RRL_FAST_BASELINES", raising=False)
    else:
        monkeypatch.setenv("RRL_FAST_BASELINES", switch)
    on = switch == "1"
    for name, flags in RECOVERY_RL.items():
        assert fast_path_supported(cfg(*flags)), name
    for name, flags in COMPARISON.items():
        assert fast_path_supported(cfg(*flags)) == on, name
    for name, flags in NEVER.items():
        assert not fast_path_supported(cfg(*flags)), name
        assert not fast_path_supported(cfg(*(flags + COMPARISON["LR"]))), name
    c = cfg(*COMPARISON["RCPO"])
    c.cnn = True
    assert not fast_path_supported(c)
