#!/usr/bin/env python3
"""Generate tests/golden/heuristic_weights.json from the reference implementation.

The reference's HeuristicAgent with weights of its own (agents/heuristic_agent.py
set_weights, the arena's params["weights"]: analytics/tournament/arena_runner.py:423-428):

* ``scores``: the per-move scores (float hex) of a few tests/golden/positions.json
  positions under each weight set -- pins the host scorer with non-default weights;
* ``games``: four full games of four HeuristicAgents, each seat another set -- one game per
  rotation of the seat-to-set map, so every (seat, set) pair is played -- from the empty
  board (trace, scores, winners, passes, turns, each seat's final RNG position and state
  hash) -- replayed through bk_rollout_frontier_w;
* ``arena_pure`` / ``arena_mixed``: run_single_game records of a run config whose
  heuristic agents carry "weights", without and with search seats -- what
  run_games_batched must return.

Every set is inside BK_HEUR_MAX_S = 128 (S = 5|size| + 20|corner| + 5|edge| + |centre|):
A 80.65, B 10.5, C 0, D 64 (B and D are partial dicts: the other weights stay default).

Usage:  python tools/gen_heuristic_weights_fixtures.py     (CPU only; needs the reference
tree, BLOKUS_REFERENCE or /root/reference)
"""
from __future__ import annotations

import os
import sys
from multiprocessing import Pool

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_fixtures import POSITION_SPECS, _gid_map, _setup, _sha, dump, move_int  # noqa: E402

WEIGHT_SETS = {
    "A": {"piece_size": 0.3, "corner_creation": 3.7, "edge_avoidance": -0.45, "center_preference": 2.9},
    "B": {"corner_creation": 0.0, "edge_avoidance": 1.0},
    "C": {"piece_size": 0.0, "corner_creation": 0.0, "edge_avoidance": 0.0, "center_preference": 0.0},
    "D": {"piece_size": -2, "center_preference": 6.5},
}
SCORE_POSITIONS = [0, 3, 9, 20, 37, 45]  # POSITION_SPECS indices: empty board .. move 48 (early and late edge rule)
# games: (seed, the set of seat p) -- one game per rotation of the sets over the seats, so
# games side by side in a launch disagree on the set at every seat
GAMES = [(9101, ["A", "B", "C", "D"]), (9102, ["B", "C", "D", "A"]), (9103, ["C", "D", "A", "B"]),
         (9104, ["D", "A", "B", "C"])]

ARENA_PURE = {"agents": [{"name": "ha", "type": "heuristic", "params": {"weights": WEIGHT_SETS["A"]}},
                         {"name": "hb", "type": "heuristic", "params": {"weights": WEIGHT_SETS["B"]}},
                         {"name": "h", "type": "heuristic"}, {"name": "r", "type": "random"}],
              "num_games": 8, "seed": 777101, "seat_policy": "round_robin", "output_root": "/tmp/arena_hw1"}
ARENA_MIXED = {"agents": [{"name": "ha", "type": "heuristic", "params": {"weights": WEIGHT_SETS["A"]}},
                          {"name": "hd", "type": "heuristic", "params": {"weights": WEIGHT_SETS["D"]}},
                          {"name": "m", "type": "mcts", "params": {"iterations": 3, "max_rollout_moves": 2}},
                          {"name": "f", "type": "fast_mcts", "params": {"time_limit": 0.01}}],
               "num_games": 4, "seed": 777102, "seat_policy": "round_robin", "output_root": "/tmp/arena_hw2"}


def _agent(seed, name):
    from agents.heuristic_agent import HeuristicAgent
    agent = HeuristicAgent(seed=seed)
    agent.set_weights(WEIGHT_SETS[name])
    return agent


def _score_case(pos):
    _setup()
    from engine.move_generator import get_shared_generator
    from tests.utils_game_states import generate_random_valid_state
    gid_of = _gid_map()
    board, cur = generate_random_valid_state(*POSITION_SPECS[pos])
    legal = get_shared_generator().get_legal_moves(board, cur)
    rec = {"position": pos, "player": cur.value, "move_count": board.move_count,
           "moves": [move_int(gid_of, m) for m in legal], "scores": {}}
    for name in WEIGHT_SETS:
        agent = _agent(1, name)
        rec["scores"][name] = [float(agent._evaluate_move(board, cur, m)).hex() for m in legal]
    return rec


def _game(job):
    """A full game of four HeuristicAgents, seat p with set seat_sets[p], from the empty
    board (arena loop semantics), as gen_fixtures._heur_game plays the default weights."""
    gseed, seat_sets = job
    _setup()
    from engine.board import Player
    from engine.game import BlokusGame
    gid_of = _gid_map()
    game = BlokusGame(enable_telemetry=False)
    agents = {p: _agent(gseed + p.value, seat_sets[p.value - 1]) for p in Player}
    trace, passes, turns = [], 0, 0
    while not game.is_game_over() and turns < 2500:
        p = game.get_current_player()
        lm = game.get_legal_moves(p)
        turns += 1
        if not lm:
            passes += 1
            trace.append(-1)
            game.board._update_current_player()
            game._check_game_over()
            continue
        mv = agents[p].select_action(game.board, p, lm)
        trace.append(move_int(gid_of, mv))
        assert game.make_move(mv, p)
    res = game.get_game_result()
    return {"seed": gseed, "seat_sets": seat_sets, "trace": trace,
            "scores": [int(res.scores[p.value]) for p in Player], "winner_ids": list(res.winner_ids),
            "passes": passes, "turns": turns,
            "rng": {p.value: [int(agents[p].rng.get_state()[2]), _sha(int(x) for x in agents[p].rng.get_state()[1])]
                    for p in Player}}


def _arena_game(job):
    config, gi = job
    _setup()
    from analytics.tournament.arena_runner import (RunConfig, _seat_assignment_for_game, game_seed_from_run_seed,
                                                   run_single_game)
    cfg = RunConfig.from_dict(config)
    gs = game_seed_from_run_seed(cfg.seed, gi)
    seats = _seat_assignment_for_game([a.name for a in cfg.agents], gi, gs, cfg.seat_policy)
    rec, _ = run_single_game(run_id="hw", game_index=gi, game_seed=gs, run_config=cfg, seat_assignment=seats,
                             agent_configs={a.name: a for a in cfg.agents})
    keep = ("game_index", "game_seed", "seat_assignment", "winner_ids", "final_scores", "moves_made",
            "turn_count", "passes", "invalid_actions", "is_tie", "error")
    return {k: rec[k] for k in keep}


def main():
    with Pool(8) as pool:
        scores = pool.map(_score_case, SCORE_POSITIONS)
        games = pool.map(_game, GAMES)
        pure = pool.map(_arena_game, [(ARENA_PURE, gi) for gi in range(ARENA_PURE["num_games"])])
        mixed = pool.map(_arena_game, [(ARENA_MIXED, gi) for gi in range(ARENA_MIXED["num_games"])])
    dump("heuristic_weights.json", {"weight_sets": WEIGHT_SETS, "scores": scores, "games": games,
                                    "arena_pure_config": ARENA_PURE, "arena_pure": pure,
                                    "arena_mixed_config": ARENA_MIXED, "arena_mixed": mixed})


if __name__ == "__main__":
    main()
