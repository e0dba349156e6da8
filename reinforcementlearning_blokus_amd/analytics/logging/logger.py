"""StrategyLogger on the GPU (reference: analytics/logging/logger.py).

``on_step`` has the reference's signature and writes the reference's ``steps.jsonl`` lines;
the board work behind a line -- eight legal-move generations and the grid scans -- is one
block of a bk_step_metrics launch (analytics.metrics).  ``batch_steps`` sets how many
captured steps one launch turns into lines: 1 (the default) puts the line on disk before
``on_step`` returns, as in the reference; a larger value packs the pair of boards at capture
(boards are mutable) and writes the pending lines, in order, when the batch is full, on
``flush()`` and on ``on_game_end``: a logger with ``batch_steps > 1`` that is dropped without
either leaves its last ``pending`` steps unwritten.
"""
from __future__ import annotations

import os
import time
from typing import Any, Dict, List, Optional

import numpy as np

from ...engine.board import Board, Player, pack_fsets, pack_states
from ..metrics import _opponents, metrics_from_step_record, pack_step
from .schemas import GameResultLog, StepLog


class StrategyLogger:
    def __init__(self, log_dir: str = "logs/analytics", *, batch_steps: int = 1, engine=None):
        """engine: anything with BlokusGPU.step_metrics' signature (default: the shared engine
        of device 0, created at the first launch)."""
        if batch_steps < 1:
            raise ValueError("batch_steps must be >= 1")
        self.log_dir = log_dir
        os.makedirs(log_dir, exist_ok=True)
        self.steps_path = os.path.join(log_dir, "steps.jsonl")
        self.results_path = os.path.join(log_dir, "results.jsonl")
        self.batch_steps = int(batch_steps)
        self.current_game_id: Optional[str] = None
        self.current_seed: Optional[int] = None
        self.agent_map: Dict[int, str] = {}
        self._engine = engine
        self._pending: List[Dict[str, Any]] = []

    # ------------------------------------------------------------------ files
    @staticmethod
    def _append(path: str, item) -> None:
        with open(path, "a") as fh:
            fh.write(f"{item.model_dump_json()}\n")

    def log_step(self, item: StepLog):
        self._append(self.steps_path, item)

    def log_result(self, item: GameResultLog):
        self._append(self.results_path, item)

    @property
    def pending(self) -> int:
        """Captured steps that have no line yet (always 0 with batch_steps=1)."""
        return len(self._pending)

    # ------------------------------------------------------------------ hooks
    def on_reset(self, game_id: str, seed: int, agent_ids: Dict[int, str], config: Dict[str, Any]):
        """A new game: its seed goes into every line, its agent names into the result line."""
        self.current_game_id, self.current_seed, self.agent_map = game_id, seed, dict(agent_ids)

    def on_step(self, game_id: str, turn_index: int, player_id: int, state: Board, move, next_state: Board):
        used = next_state.player_pieces_used.get(Player(player_id), set())
        self._pending.append({
            "game_id": game_id, "timestamp": time.time(), "seed": self.current_seed,
            "turn_index": turn_index, "player_id": player_id,
            "action": {"piece_id": move.piece_id, "orientation": move.orientation, "anchor_row": move.anchor_row,
                       "anchor_col": move.anchor_col},
            "pieces_remaining": [i for i in range(1, 22) if i not in used],
            "packed": (pack_states([state]), pack_fsets([state]), pack_states([next_state]), pack_fsets([next_state]),
                       pack_step(player_id, move)),
        })
        if len(self._pending) >= self.batch_steps:
            self.flush()

    def flush(self):
        """One launch for the captured steps; their lines are written in capture order.  No
        captured step is lost without a word: if the launch itself raises, every step stays
        pending; if a record carries a status bit, the lines before that step are written, that
        step is dropped, the steps after it stay pending for the next flush, and the error
        names the dropped step."""
        pending = self._pending
        if not pending:
            return
        if self._engine is None:
            from ...gpu import BlokusGPU
            self._engine = BlokusGPU.shared(0)
        recs = self._engine.step_metrics(*(np.concatenate([p["packed"][k] for p in pending]) for k in range(5)))
        for done, (p, rec) in enumerate(zip(pending, recs)):
            pid, turn = p["player_id"], p["turn_index"]
            if int(rec["status"]):
                self._pending = pending[done + 1:]
                raise RuntimeError(f"bk_step_metrics: status {int(rec['status'])} for game_id {p['game_id']!r}, "
                                   f"turn_index {turn}: the step does not describe its boards; it is dropped, "
                                   f"{done} lines before it are written, {len(self._pending)} steps stay pending")
            self.log_step(StepLog(
                game_id=p["game_id"], timestamp=p["timestamp"], seed=p["seed"], turn_index=turn, player_id=pid,
                action=p["action"],
                legal_moves_before=int(rec["moves_before"][pid - 1]), legal_moves_after=int(rec["moves_after"][pid - 1]),
                pieces_remaining=p["pieces_remaining"],
                metrics=metrics_from_step_record(rec, pid, _opponents(pid), p["action"]["piece_id"]),
                round_index=turn // 4, position_in_round=turn % 4, seat_index=pid - 1))
        self._pending = []

    def on_game_end(self, game_id: str, final_scores: Dict[int, int], winner_id: Optional[int], num_turns: int):
        """Writes the pending lines, then the game's result line."""
        self.flush()
        self.log_result(GameResultLog(
            game_id=game_id, timestamp=time.time(),
            final_scores={str(pid): score for pid, score in final_scores.items()},
            winner_id=winner_id, num_turns=num_turns,
            agent_ids={str(pid): name for pid, name in self.agent_map.items()},
            seat_order=[p.value for p in Player]))
