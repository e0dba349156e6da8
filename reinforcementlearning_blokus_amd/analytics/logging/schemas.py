"""The two record types of the strategy log, with the field names and order of the reference's
analytics/logging/schemas.py (they are the JSONL format).

Keyword-only dataclasses serialised with ``json``: the package does not depend on pydantic.
``model_dump_json`` is there for callers written against the reference's models.
"""
from __future__ import annotations

import json
from dataclasses import asdict, dataclass
from typing import Any, Dict, List, Optional


class _JsonModel:
    def model_dump(self) -> Dict[str, Any]:
        return asdict(self)

    def model_dump_json(self) -> str:
        return json.dumps(asdict(self), separators=(",", ":"))


@dataclass(kw_only=True)
class StepLog(_JsonModel):
    """One line of steps.jsonl: a placement, the mover's legal-move counts around it and its 28
    metrics.  Field names and order are the file format."""
    game_id: str
    timestamp: float                                # time.time() when on_step captured the step
    seed: Optional[int]                             # the game's seed as given to on_reset
    turn_index: int                                 # placements logged before this one
    player_id: int                                  # Player.value of the mover, 1..4
    action: Dict[str, Any]                          # piece_id, orientation, anchor_row, anchor_col
    board_hash: Optional[str] = None                # never filled by StrategyLogger
    pieces_remaining: Optional[List[int]] = None    # piece ids the mover holds after the move
    legal_moves_before: int                         # bk_step_rec.moves_before of the mover
    legal_moves_after: int
    metrics: Dict[str, Any]                         # analytics.metrics.metrics_from_step_record
    round_index: Optional[int] = None               # turn_index // 4
    position_in_round: Optional[int] = None         # turn_index % 4
    seat_index: Optional[int] = None                # player_id - 1


@dataclass(kw_only=True)
class GameResultLog(_JsonModel):
    """The one line of results.jsonl a finished game gets."""
    game_id: str
    timestamp: float
    final_scores: Dict[str, int]  # by Player.value written as a string (JSON object keys)
    winner_id: Optional[int]      # None for a tie
    num_turns: int                # placements logged
    agent_ids: Dict[str, str]     # Player.value as a string -> the name given to on_reset
    seat_order: List[int]
