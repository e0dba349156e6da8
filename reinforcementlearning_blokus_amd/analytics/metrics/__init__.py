"""Per-move strategy metrics (reference: analytics/metrics/).

The reference derives its 28 move metrics from eight legal-move generations (four players,
before and after the move) and numpy scans of the two grids.  Here one bk_step_metrics
launch (gpu.BlokusGPU.step_metrics, k_steplog) returns the integers behind all of them for
any number of steps, and ``metrics_from_step_record`` turns one record into the reference's
dicts with host arithmetic in the reference's order: every float is one division of two
integers, so it equals CPython's.  The seven ``compute_*`` functions keep the reference's
signatures; on one ``MetricInput`` the first that needs board work makes the launch and
caches the record in ``inp.precomputed_values``.  There is no CPU implementation of the
board work behind this module.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..._native import STEP_DTYPE, STEP_REC_DTYPE
from ...engine.board import Board, Player, pack_fsets, pack_states
from ...engine.pieces import GID, ORIENT_CELLS, PieceGenerator

BOARD_SIZE = 20
CENTER_COORD = ((BOARD_SIZE - 1) / 2, (BOARD_SIZE - 1) / 2)
CENTER_MASK_RADIUS_K = 4
RECORD_KEY = "step_record"  # the cached bk_step_rec in MetricInput.precomputed_values


def mdist(pos1: Tuple[float, float], pos2: Tuple[float, float]) -> float:
    """|row difference| + |column difference| of two cells."""
    return abs(pos1[0] - pos2[0]) + abs(pos1[1] - pos2[1])


def is_in_center_mask(pos: Tuple[int, int], k: int = CENTER_MASK_RADIUS_K) -> bool:
    return mdist(pos, CENTER_COORD) <= k


@dataclass
class MetricInput:
    """What the seven compute_* functions take: one placement and the boards around it.

    The board work comes from a bk_step_metrics launch on (state, move, next_state), which
    differs from the reference in two places, both checked, neither silent: the placed cells
    are ``move``'s cells from the orientation table, so ``placed_squares``, when given and not
    empty, must be exactly those cells (``ValueError`` otherwise, from the center and
    proximity functions); and the distance to the opponents is measured to every cell that
    is not the mover's, so ``compute_proximity_metrics`` needs ``opponents`` to be the three
    other players (``ValueError`` otherwise).  The mobility, blocking and corner functions
    take any subset of opponents, in the order given."""
    state: Any       # this package's Board before the move
    move: Any        # Move (piece_id, orientation, anchor_row, anchor_col)
    next_state: Any  # this package's Board after the move
    player_id: int   # the mover's Player.value
    opponents: List[int]

    placed_squares: Optional[List[Tuple[int, int]]] = None  # (row, col) of the cells the move covers
    precomputed_values: Optional[Dict[str, Any]] = None     # mobility counts and the cached record

    def get_placed_squares(self) -> List[Tuple[int, int]]:
        if self.placed_squares is not None:
            return self.placed_squares
        return []


def _shape_perimeter(mask: np.ndarray) -> int:
    padded = np.pad(mask.astype(int), 1, mode="constant", constant_values=0)
    return int(np.sum(np.abs(np.diff(padded, axis=0))) + np.sum(np.abs(np.diff(padded, axis=1))))


# piece id -> (size, perimeter of the base shape), from engine/pieces.py
PIECE_TABLE: Dict[int, Tuple[int, int]] = {p.id: (int(p.size), _shape_perimeter(p.shape))
                                           for p in PieceGenerator.get_all_pieces()}
assert len(PIECE_TABLE) == 21


# ------------------------------------------------------------------ records
def _engine():
    from ...gpu import BlokusGPU
    return BlokusGPU.shared(0)


def pack_step(player_id: int, move) -> np.ndarray:
    """One bk_step (STEP_DTYPE[1]) of a mover's Player.value and a Move."""
    s = np.zeros(1, dtype=STEP_DTYPE)
    s["mover"] = int(player_id) - 1
    s["piece_id"], s["orientation"] = int(move.piece_id), int(move.orientation)
    s["anchor_row"], s["anchor_col"] = int(move.anchor_row), int(move.anchor_col)
    return s


def check_record(rec, where: str = "") -> None:
    if int(rec["status"]):
        raise RuntimeError(f"bk_step_metrics: the step{where} does not describe its boards or their frontier "
                           f"tables are invalid (status {int(rec['status'])})")


def step_records(states: Sequence[Board], next_states: Sequence[Board], player_ids: Sequence[int], moves: Sequence,
                 engine=None) -> np.ndarray:
    """The bk_step_rec records (STEP_REC_DTYPE[n]) of n steps, all in ONE launch.  The status
    is left to the caller (check_record)."""
    n = len(states)
    if not (len(next_states) == len(player_ids) == len(moves) == n):
        raise ValueError("step_records: states, next_states, player_ids and moves differ in length")
    if n == 0:
        return np.zeros(0, dtype=STEP_REC_DTYPE)
    steps = np.concatenate([pack_step(pid, mv) for pid, mv in zip(player_ids, moves)])
    eng = engine if engine is not None else _engine()
    return eng.step_metrics(pack_states(states), pack_fsets(states), pack_states(next_states), pack_fsets(next_states),
                            steps)


def _opponents(player_id: int) -> List[int]:
    return [p.value for p in Player if p.value != player_id]


def step_metrics_many(states: Sequence[Board], next_states: Sequence[Board], player_ids: Sequence[int],
                      moves: Sequence, engine=None) -> List[Dict[str, Any]]:
    """The 28 metrics of every step (the logger's merged dict), all steps in ONE launch."""
    recs = step_records(states, next_states, player_ids, moves, engine)
    out = []
    for i, (rec, pid, mv) in enumerate(zip(recs, player_ids, moves)):
        check_record(rec, f" {i}")
        out.append(metrics_from_step_record(rec, int(pid), _opponents(int(pid)), mv.piece_id))
    return out


# ------------------------------------------------------------------ host arithmetic
def _counts(rec, players: Sequence[int]) -> Tuple[Dict[int, int], Dict[int, int]]:
    return ({p: int(rec["moves_before"][p - 1]) for p in players},
            {p: int(rec["moves_after"][p - 1]) for p in players})


def _center(rec) -> Dict[str, Any]:
    n = int(rec["placed_cells"])
    if n == 0:
        return {"center_distance": 0.0, "center_gain": 0}
    return {"center_distance": float(int(rec["center_dist_sum"])) / n, "center_gain": int(rec["center_gain"])}


def _territory(rec) -> Dict[str, Any]:
    area_after, perim_after = int(rec["area_after"]), int(rec["perimeter_after"])
    bbox = int(rec["bbox_area_after"])
    return {"area_gain": area_after - int(rec["area_before"]),
            "perimeter_after": perim_after,
            "delta_perimeter": perim_after - int(rec["perimeter_before"]),
            "compactness_after": area_after / (perim_after ** 2) if perim_after > 0 else 0.0,
            "bbox_fill_after": area_after / bbox if bbox > 0 else 0.0}


def _mobility(before: Dict[int, int], after: Dict[int, int], me: int, opponents: Sequence[int]) -> Dict[str, Any]:
    m_before, m_after = before.get(me, 0), after.get(me, 0)
    opp_before = sum(before.get(o, 0) for o in opponents)
    opp_after = sum(after.get(o, 0) for o in opponents)
    return {"mobility_me_before": m_before, "mobility_me_after": m_after, "mobility_me_delta": m_after - m_before,
            "mobility_me_ratio": m_after / m_before if m_before > 0 else 0.0,
            "mobility_opp_before_sum": opp_before, "mobility_opp_after_sum": opp_after,
            "mobility_opp_delta_sum": opp_after - opp_before}


def _blocking(before: Dict[int, int], after: Dict[int, int], opponents: Sequence[int], n_placed: int) -> Dict[str, Any]:
    blocking, max_loss, target = 0, -1, None
    for o in opponents:  # the first opponent with the strictly greatest loss
        loss = max(0, before.get(o, 0) - after.get(o, 0))
        blocking += loss
        if loss > max_loss:
            max_loss, target = loss, o
    return {"blocking": blocking, "block_eff": blocking / max(1, n_placed), "blocking_target_id": target,
            "blocking_target_loss": max_loss if target is not None else 0}


def _corners(rec, me: int, opponents: Sequence[int]) -> Dict[str, Any]:
    fb = [int(x) for x in rec["frontier_before"]]
    fa = [int(x) for x in rec["frontier_after"]]
    return {"corners_me_before": fb[me - 1], "corners_me_after": fa[me - 1],
            "corners_me_delta": fa[me - 1] - fb[me - 1],
            "corners_opp_before_sum": sum(fb[o - 1] for o in opponents),
            "corners_opp_after_sum": sum(fa[o - 1] for o in opponents),
            "corner_block": sum(max(0, fb[o - 1] - fa[o - 1]) for o in opponents)}


def _proximity(rec) -> Dict[str, Any]:
    if int(rec["placed_cells"]) == 0:
        return {"dist_to_opp_min": float(BOARD_SIZE * 2), "is_close_3": 0}
    d = int(rec["dist_to_opp_min"])
    return {"dist_to_opp_min": float(d), "is_close_3": 1 if d <= 3 else 0}


def _piece(piece_id) -> Dict[str, Any]:
    size, complexity = PIECE_TABLE.get(piece_id, (0, 0)) if piece_id is not None else (0, 0)
    return {"piece_size": size, "piece_complexity": complexity}


def metrics_from_step_record(rec, player_id: int, opponents: Sequence[int], piece_id) -> Dict[str, Any]:
    """One bk_step_rec (a numpy record or any mapping with its field names) as the 28 metrics
    of a StepLog line, in the logger's order: center, territory, mobility, blocking, corners,
    proximity, piece.  player_id and opponents are Player values.  Host arithmetic only."""
    before, after = _counts(rec, [player_id, *opponents])
    out: Dict[str, Any] = {}
    out.update(_center(rec))
    out.update(_territory(rec))
    out.update(_mobility(before, after, player_id, opponents))
    out.update(_blocking(before, after, opponents, int(rec["placed_cells"])))
    out.update(_corners(rec, player_id, opponents))
    out.update(_proximity(rec))
    out.update(_piece(piece_id))
    return out


# ------------------------------------------------------------------ the reference's functions
def _record(inp: MetricInput):
    """The step's record: from inp.precomputed_values, or one launch that leaves it there."""
    if inp.precomputed_values is None:
        inp.precomputed_values = {}
    rec = inp.precomputed_values.get(RECORD_KEY)
    if rec is None:
        rec = step_records([inp.state], [inp.next_state], [inp.player_id], [inp.move])[0]
        check_record(rec)
        inp.precomputed_values[RECORD_KEY] = rec
    return rec


def _placed_cells(inp: MetricInput) -> List[Tuple[int, int]]:
    """inp.placed_squares, after checking that they are the cells of inp.move (the cells the
    launch works on)."""
    placed = inp.get_placed_squares()
    mv = inp.move
    g = GID.get((getattr(mv, "piece_id", None), getattr(mv, "orientation", None)))
    if g is None:
        raise ValueError(f"MetricInput.move is no placement: {mv!r}")
    cells = sorted((mv.anchor_row + r, mv.anchor_col + c) for r, c in ORIENT_CELLS[g])
    if sorted((int(r), int(c)) for r, c in placed) != cells:
        raise ValueError(f"MetricInput.placed_squares {sorted(placed)} are not the cells of {mv}: {cells}")
    return placed


def get_mobility_counts(inp: MetricInput) -> Tuple[Dict[int, int], Dict[int, int]]:
    """The legal-move counts before and after the move by player id; caller-supplied
    ``mobility_counts_before`` / ``mobility_counts_after`` in inp.precomputed_values win."""
    pre = inp.precomputed_values or {}
    before, after = pre.get("mobility_counts_before"), pre.get("mobility_counts_after")
    if before is None or after is None:
        got_before, got_after = _counts(_record(inp), [inp.player_id, *inp.opponents])
        before = got_before if before is None else before
        after = got_after if after is None else after
    return before, after


def compute_center_metrics(inp: MetricInput) -> Dict[str, Any]:
    """Over the cells of inp.move; inp.placed_squares must be those cells, or empty (the
    reference's zeros, no launch)."""
    if not inp.get_placed_squares():
        return {"center_distance": 0.0, "center_gain": 0}
    _placed_cells(inp)
    return _center(_record(inp))


def compute_territory_metrics(inp: MetricInput) -> Dict[str, Any]:
    return _territory(_record(inp))


def compute_mobility_metrics(inp: MetricInput) -> Dict[str, Any]:
    before, after = get_mobility_counts(inp)
    return _mobility(before, after, inp.player_id, inp.opponents)


def compute_blocking_metrics(inp: MetricInput) -> Dict[str, Any]:
    before, after = get_mobility_counts(inp)
    return _blocking(before, after, inp.opponents, len(inp.get_placed_squares()))


def compute_corner_metrics(inp: MetricInput) -> Dict[str, Any]:
    return _corners(_record(inp), inp.player_id, inp.opponents)


def compute_proximity_metrics(inp: MetricInput) -> Dict[str, Any]:
    """From the cells of inp.move to every cell of the before board that is not the mover's:
    inp.opponents must be the three other players and inp.placed_squares the move's cells, or
    empty (the reference's 40.0, no launch)."""
    if not inp.get_placed_squares():
        return {"dist_to_opp_min": float(BOARD_SIZE * 2), "is_close_3": 0}
    _placed_cells(inp)
    if sorted(inp.opponents) != _opponents(inp.player_id):
        raise ValueError(f"compute_proximity_metrics: opponents {inp.opponents} are not the three other players "
                         f"of player {inp.player_id}; the kernel measures to every cell that is not the mover's")
    return _proximity(_record(inp))


def compute_piece_metrics(inp: MetricInput) -> Dict[str, Any]:
    return _piece(getattr(inp.move, "piece_id", None))


__all__ = [
    "BOARD_SIZE", "CENTER_COORD", "CENTER_MASK_RADIUS_K", "MetricInput", "mdist", "is_in_center_mask",
    "compute_center_metrics", "compute_territory_metrics", "compute_mobility_metrics", "compute_blocking_metrics",
    "compute_corner_metrics", "compute_proximity_metrics", "compute_piece_metrics", "get_mobility_counts",
    "metrics_from_step_record", "step_metrics_many", "step_records", "pack_step", "check_record", "PIECE_TABLE",
]
