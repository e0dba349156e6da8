"""The strategy step log (reference: analytics/logging/ and the game loop of
scripts/generate_analytics_data.py)."""
from __future__ import annotations

from ...engine.board import Player
from .logger import StrategyLogger
from .reader import load_jsonl, load_steps_for_game, resolve_steps_path
from .schemas import GameResultLog, StepLog


def run_game_with_logging(game_id, agents, logger, seed=42):
    """Play one game of ``agents`` ({Player: agent}) and log every placement: a copy of the
    board before the move, ``logger.on_step`` after a successful ``make_move``, a pass when the
    current player has no move, ``logger.on_game_end`` at the end.  Returns the GameResult."""
    from ...engine.game import BlokusGame
    game = BlokusGame(enable_telemetry=False)
    logger.on_reset(game_id, seed, {p.value: f"{type(agents[p]).__name__}_{p.name}" for p in Player}, {})
    turn_index = 0
    while not game.is_game_over():
        player = game.get_current_player()
        before = game.get_board_copy()
        legal = game.get_legal_moves(player)
        move = agents[player].select_action(game.board, player, legal) if legal else None
        if move is None:  # a pass
            game.board._update_current_player()
            game._check_game_over()
            continue
        if game.make_move(move, player):
            logger.on_step(game_id, turn_index, player.value, before, move, game.board)
            turn_index += 1
    res = game.get_game_result()
    logger.on_game_end(game_id, res.scores, res.winner_ids[0] if not res.is_tie else None, turn_index)
    return res


__all__ = ["StrategyLogger", "StepLog", "GameResultLog", "load_jsonl", "resolve_steps_path", "load_steps_for_game",
           "run_game_with_logging"]
