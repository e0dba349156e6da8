"""Readers of StrategyLogger's JSONL files (reference: analytics/logging/reader.py).

Two layouts: one directory per game, ``{base}/{sanitised game id}/steps.jsonl``, and the
flat ``{base}/steps.jsonl`` holding every game, filtered by ``game_id``.  Host only.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional, Tuple

_KEPT = frozenset("_-")


def _sanitize_game_id(game_id: str) -> str:
    """A game id as a directory name: everything but alphanumerics, ``_`` and ``-`` becomes ``_``."""
    return "".join(ch if (ch.isalnum() or ch in _KEPT) else "_" for ch in game_id)


def load_jsonl(path: str, filter_game_id: Optional[str] = None) -> List[Dict[str, Any]]:
    """The objects of a JSONL file, in file order; blank lines and lines that are not JSON are
    skipped, a missing file is an empty list.  With filter_game_id only that game's objects."""
    if not os.path.exists(path):
        return []
    rows: List[Dict[str, Any]] = []
    with open(path) as fh:
        for raw in fh:
            if not raw.strip():
                continue
            try:
                row = json.loads(raw)
            except json.JSONDecodeError:
                continue
            if filter_game_id is None or row.get("game_id") == filter_game_id:
                rows.append(row)
    return rows


def resolve_steps_path(base_dir: str, game_id: str) -> Tuple[str, Optional[str]]:
    """(per-game path, flat path) of a game's steps; the flat path is None when it is the same file."""
    per_game = os.path.join(base_dir, _sanitize_game_id(game_id), "steps.jsonl")
    flat = os.path.join(base_dir, "steps.jsonl")
    return per_game, (None if flat == per_game else flat)


def load_steps_for_game(base_dir: str, game_id: str) -> List[Dict[str, Any]]:
    """A game's StepLog entries by (turn_index, timestamp): the per-game file if it holds any,
    else the flat file's entries of that game."""
    per_game, flat = resolve_steps_path(base_dir, game_id)
    rows = load_jsonl(per_game)
    if not rows and flat:
        rows = load_jsonl(flat, filter_game_id=game_id)
    return sorted(rows, key=lambda row: (row.get("turn_index", 0), row.get("timestamp", 0)))
