"""MCTSAgent's ``rollout_backend="leaf"`` without a GPU: the option rules, the C-ABI surface
(bk_mcts_learned exported within ABI 7, struct sizes unchanged) and search_packed's grouping
of leaf agents with the launch stubbed."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from reinforcementlearning_blokus_amd.mcts.mcts_agent import MCTSAgent
from tests.conftest import load_golden

FIX = load_golden("winprob_eval.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    path = tmp_path_factory.mktemp("leaf_host") / "model.json"
    path.write_text(json.dumps(FIX["model"]))
    return str(path)


def leaf(model_path, **kw):
    kw.setdefault("leaf_evaluation_enabled", True)
    kw.setdefault("learned_model_path", model_path)
    return MCTSAgent(iterations=24, rollout_backend="leaf", **kw)


def test_option_rules(model_path, tmp_path):
    agent = leaf(model_path, progressive_bias_enabled=True, seed=3)
    assert agent.rollout_backend == "leaf" and agent.learned_evaluator.model_type == "pairwise_logreg"
    assert agent.get_action_info()["parameters"]["rollout_backend"] == "leaf"
    assert leaf(model_path, rollout_agent=None).rollout_backend == "leaf"  # no rollout agent needed
    with pytest.raises(ValueError, match="potential shaping needs rollouts; use rollout_backend='exact'"):
        leaf(model_path, potential_shaping_enabled=True)
    with pytest.raises(ValueError, match="only together with leaf evaluation; use rollout_backend='exact'"):
        leaf(model_path, leaf_evaluation_enabled=False, progressive_bias_enabled=True)
    with pytest.raises(ValueError, match="needs leaf_evaluation_enabled=True"):
        leaf(model_path, leaf_evaluation_enabled=False)
    with pytest.raises(ValueError, match="learned_model_path is required"):
        leaf(None)
    with pytest.raises(ValueError, match="weight of 0 .* use rollout_backend='exact'"):
        leaf(model_path, progressive_bias_enabled=True, progressive_bias_weight=0.0)
    dummy = tmp_path / "dummy_model.json"
    dummy.write_text("{}")
    with pytest.raises(ValueError, match="dummy evaluator; use rollout_backend='exact'"):
        leaf(str(dummy))
    gbt = tmp_path / "gbt.json"
    gbt.write_text(json.dumps(dict(FIX["model"], model_type="pairwise_gbt_phase")))
    with pytest.raises(ValueError, match="pairwise_gbt_phase.*rollout_backend='exact'"):
        leaf(str(gbt))
    with pytest.raises(ValueError, match="must be 'search', 'exact', 'kernel' or 'leaf'"):
        MCTSAgent(iterations=4, rollout_backend="tree")


def test_existing_backends_keep_their_rules(model_path):
    for backend in ("search", "kernel"):
        with pytest.raises(ValueError, match="does not evaluate leaves"):
            MCTSAgent(iterations=4, learned_model_path=model_path, leaf_evaluation_enabled=True,
                      rollout_backend=backend)
    for options in ({"leaf_evaluation_enabled": True}, {"progressive_bias_enabled": True},
                    {"potential_shaping_enabled": True}, {}):
        assert MCTSAgent(iterations=4, learned_model_path=model_path, **options).rollout_backend == "exact"
    assert MCTSAgent(iterations=4, seed=3).rollout_backend == "search"


def test_arena_config_forwards_the_backend(model_path):
    from reinforcementlearning_blokus_amd.arena.config import AgentConfig
    from reinforcementlearning_blokus_amd.arena.runner import build_agent
    cfg = AgentConfig(name="m", type="mcts", params={"iterations": 8, "learned_model_path": model_path,
                                                     "leaf_evaluation_enabled": True, "rollout_backend": "leaf"})
    assert build_agent(cfg, 5).agent.rollout_backend == "leaf"
    cfg = AgentConfig(name="m", type="mcts", params={"iterations": 8, "learned_model_path": model_path,
                                                     "leaf_evaluation_enabled": True})
    assert build_agent(cfg, 5).agent.rollout_backend == "exact"


def test_abi_surface():
    assert N.ABI_VERSION == 7 and "bk_mcts_learned" in N.EXPORTS
    assert N.DIAG_KERNELS[5] == "k_mcts_coop_l" and N.DIAG_KERNELS[:5] == ("k_mcts", "k_mcts_pair", "k_mcts_h",
                                                                            "k_mcts_coop", "k_mcts_coop_h")
    header = open(os.path.join(ROOT, "include", "blokus_hip.h")).read()
    assert re.search(r"#define BK_ABI_VERSION 7\b", header) and re.search(r"#define BK_DIAG_K_COOP_L 5\b", header)
    decl = re.search(r"int bk_mcts_learned\(([^;]*)\);", header).group(1)
    assert "mt_state" not in decl and "const bk_winprob_model* model" in decl and "double* prior_bias" in decl
    assert decl.count(",") + 1 == 25  # the handle, 23 arguments and the memory mode, as the binding declares
    # the records a launch exchanges are unchanged
    assert (N.MCTS_NODE_DTYPE.itemsize, N.MCTS_OUT_DTYPE.itemsize, ctypes.sizeof(N.BkMctsCfg)) == (24, 32, 48)
    assert ctypes.sizeof(N.BkWinprobModel) == 8 * (3 * 34 + 1) and N.STATE_DTYPE.itemsize == 256
    assert re.search(r"\} bk_mcts_node;\s*/\* 24 bytes \*/", header)
    lib = N.LIB_PATH
    if os.path.exists(lib):  # built: the symbol is there and the library still reports ABI 7
        L = ctypes.CDLL(lib)
        assert L.bk_abi_version() == 7 and hasattr(L, "bk_mcts_learned")
        for name in N.EXPORTS:
            assert hasattr(L, name), name


def test_search_packed_groups_leaf_agents(model_path, tmp_path, monkeypatch):
    other = tmp_path / "other.json"
    other.write_text(json.dumps(dict(FIX["model"], intercept=repr(float(FIX["model"]["intercept"]) + 0.5))))
    agents = [leaf(model_path, seed=1), leaf(model_path, seed=2), leaf(str(other), seed=3),
              leaf(model_path, seed=4, progressive_bias_enabled=True),
              leaf(model_path, seed=5, use_transposition_table=False)]
    assert agents[0].learned_evaluator.model is not agents[1].learned_evaluator.model  # grouped by value
    calls = []

    def fake_leaf(agents_, roots, sets, players, key, idx, out):
        calls.append((key, list(idx)))
        for i in idx:
            out[i] = 1000 + i

    monkeypatch.setattr(MCTSAgent, "_leaf_group", staticmethod(fake_leaf))
    roots = np.zeros(len(agents), dtype=N.STATE_DTYPE)
    sets = np.zeros(len(agents), dtype=N.FSET_DTYPE)
    got = MCTSAgent.search_packed(agents, roots, sets, [0, 1, 2, 3, 0])
    assert got == [1000, 1001, 1002, 1003, 1004]
    groups = sorted(idx for _, idx in calls)
    assert groups == [[0, 1], [2], [3], [4]]  # two models, bias on / off and TT on / off: four launches
    for key, idx in calls:
        assert key[0] == "leaf" and key[1] == 24 and key[6] == 2500
        assert key[7] == (0.25 if idx == [3] else 0.0) and key[3] == (idx != [4])
    with pytest.raises(ValueError, match="'search' or 'leaf' agents"):
        MCTSAgent.search_packed([MCTSAgent(iterations=4, learned_model_path=model_path)], roots[:1], sets[:1], [0])
