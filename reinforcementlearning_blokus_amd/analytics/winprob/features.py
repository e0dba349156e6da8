"""Feature extraction for win-probability modelling (reference: analytics/winprob/features.py).

One row of 34 features per player and snapshot.  The board work behind a row -- four legal
move generations, the board-wide dead-zone fill, the centre and adjacency scans -- runs in
one bk_snapshot_features launch (gpu.BlokusGPU.snapshot_features) for any number of boards.
The launch returns the integers (``SNAPSHOT_REC_DTYPE`` records) and the finished rows as
doubles computed on the device; ``features_from_record`` builds the same row from a record
with host arithmetic in the reference's order, so both equal CPython's floats bit for bit.
There is no CPU implementation of the board work behind this module.
"""
from __future__ import annotations

from collections.abc import Iterable, Mapping
from dataclasses import dataclass
from typing import Any, Dict, List, Sequence

from ...engine.board import Board, Player, pack_fsets, pack_states
from ...engine.mobility_metrics import mobility_from_counts, piece_tables

SNAPSHOT_FEATURE_COLUMNS: List[str] = [
    "frontier_size",
    "corner_differential",
    "center_proximity",
    "opponent_adjacency",
    "deadzone_count",
    "deadzone_fraction",
    "mobility_total_placements",
    "mobility_total_orientation_normalized",
    "mobility_total_cell_weighted",
    "mobility_bucket_1",
    "mobility_bucket_2",
    "mobility_bucket_3",
    "mobility_bucket_4",
    "mobility_bucket_5",
    "blocking_exposure_legal_moves_opp_sum",
    "utility_frontier_plus_mobility",
    "pieces_used_count",
    "pieces_remaining_count",
    "remaining_squares",
    "remaining_size_1_count",
    "remaining_size_2_count",
    "remaining_size_3_count",
    "remaining_size_4_count",
    "remaining_size_5_count",
    "remaining_key_piece_17",
    "remaining_key_piece_19",
    "remaining_key_piece_20",
    "phase_ply",
    "phase_turn_index",
    "phase_board_occupancy",
    "phase_piece_usage_ratio",
    "phase_progress_turn_ratio",
    "phase_progress_placement_ratio",
    "player_board_occupancy",
]

_PLAYERS = list(Player)
_BOARD_CELLS = Board.SIZE * Board.SIZE


@dataclass(frozen=True)
class SnapshotRuntimeContext:
    """Context values reused across all players at one snapshot."""

    ply: int
    turn_index: int
    board_occupancy: float
    deadzone_count: int
    deadzone_fraction: float
    progress_turn_ratio: float
    progress_placement_ratio: float


def _engine(move_generator=None):
    if move_generator is not None and hasattr(move_generator, "_engine"):
        return move_generator._engine()
    from ...gpu import BlokusGPU
    return BlokusGPU.shared(getattr(move_generator, "device", 0))


def _check(rec) -> None:
    if int(rec["status"]):
        raise RuntimeError(f"bk_snapshot_features: the position or its frontier tables are invalid "
                           f"(status {int(rec['status'])})")


def _records(board: Board, turn_index: int, max_turns: int, move_generator=None):
    """The four players' records of one board (one launch, no feature matrix)."""
    recs, _ = _engine(move_generator).snapshot_features(pack_states([board]), pack_fsets([board]), [int(turn_index)],
                                                        int(max_turns), records=True, features=False)
    for r in recs[0]:
        _check(r)
    return recs[0]


def _context(*, ply: int, turn_index: int, max_turns: int, occupied_cells: int,
             deadzone_count: int) -> SnapshotRuntimeContext:
    """The context's floats, each one division of two integers as in the reference."""
    span = max(1, max_turns)
    return SnapshotRuntimeContext(ply=int(ply), turn_index=int(turn_index),
                                  board_occupancy=occupied_cells / _BOARD_CELLS,
                                  deadzone_count=int(deadzone_count),
                                  deadzone_fraction=deadzone_count / _BOARD_CELLS,
                                  progress_turn_ratio=turn_index / span, progress_placement_ratio=ply / span)


def build_snapshot_runtime_context(board: Board, *, turn_index: int, max_turns: int) -> SnapshotRuntimeContext:
    """Global snapshot context fields of the current board state (one launch)."""
    rec = _records(board, turn_index, max_turns)[0]
    return _context(ply=int(board.move_count), turn_index=turn_index, max_turns=max_turns,
                    occupied_cells=int(rec["occupied_cells"]), deadzone_count=int(rec["deadzone_count"]))


def _player_row(rec, pieces_used: Iterable[int], context: SnapshotRuntimeContext) -> Dict[str, float]:
    """One player's row from its record and the snapshot's context, columns in
    SNAPSHOT_FEATURE_COLUMNS order; every float is formed by the reference's operation."""
    _check(rec)
    used = sorted({int(x) for x in pieces_used})
    _, sizes = piece_tables()
    held = [pid for pid in range(1, 22) if pid not in used]
    counts = [int(c) for c in rec["piece_count"]]
    mob = mobility_from_counts({pid: counts[pid - 1] for pid in range(1, 22) if counts[pid - 1] > 0}, 0, used)
    frontier = float(int(rec["frontier_size"]))
    held_of_size = [sum(1 for pid in held if sizes[pid] == k) for k in range(1, 6)]
    row = [
        frontier,
        float(int(rec["corner_differential"])),
        float(int(rec["center_dist"])),
        float(int(rec["opponent_adjacency"])),
        float(context.deadzone_count),
        float(context.deadzone_fraction),
        float(mob.totalPlacements),
        float(mob.totalOrientationNormalized),
        float(mob.totalCellWeighted),
        *(float(mob.buckets.get(k, 0.0)) for k in range(1, 6)),
        float(int(rec["opp_moves_sum"])),
        frontier + float(mob.totalCellWeighted),
        float(len(used)),
        float(len(held)),
        float(sum(sizes.values()) - sum(sizes[pid] for pid in used)),
        *(float(n) for n in held_of_size),
        *(float(pid in held) for pid in (17, 19, 20)),
        float(context.ply),
        float(context.turn_index),
        float(context.board_occupancy),
        len(used) / 21.0,
        float(context.progress_turn_ratio),
        float(context.progress_placement_ratio),
        int(rec["own_cells"]) / _BOARD_CELLS,
    ]
    assert len(row) == len(SNAPSHOT_FEATURE_COLUMNS)
    return dict(zip(SNAPSHOT_FEATURE_COLUMNS, row))


def features_from_record(rec, pieces_used: Iterable[int], *, turn_index: int, max_turns: int,
                         move_count: int) -> Dict[str, float]:
    """One player's bk_snapshot_rec (a numpy record or any mapping with its field names) as
    the reference's feature dict.  Host arithmetic only, in the reference's order."""
    context = _context(ply=move_count, turn_index=turn_index, max_turns=max_turns,
                       occupied_cells=int(rec["occupied_cells"]), deadzone_count=int(rec["deadzone_count"]))
    return _player_row(rec, pieces_used, context)


def extract_player_snapshot_features(board: Board, *, player: Player, context: SnapshotRuntimeContext,
                                     move_generator=None) -> Dict[str, float]:
    """One player's feature vector for win-probability modelling (one launch; the other
    three players' records are dropped -- snapshot_features_many is the batched form)."""
    recs = _records(board, context.turn_index, 1, move_generator)
    return _player_row(recs[player.value - 1], board.player_pieces_used[player], context)


def snapshot_features_many(boards: Sequence[Board], turn_indices: Sequence[int], max_turns: int, *,
                           move_generator=None) -> List[Dict[str, Dict[str, float]]]:
    """[{Player.name: feature dict}] for every board, all of them in ONE launch; the rows
    are the device's doubles (equal to features_from_record's)."""
    boards = list(boards)
    turns = [int(t) for t in turn_indices]
    if len(turns) != len(boards):
        raise ValueError(f"turn_indices: {len(turns)} entries for {len(boards)} boards")
    if not boards:
        return []
    recs, feats = _engine(move_generator).snapshot_features(pack_states(boards), pack_fsets(boards), turns,
                                                            int(max_turns))
    return rows_from_launch(recs, feats)


def rows_from_launch(recs, feats) -> List[Dict[str, Dict[str, float]]]:
    """snapshot_features' host outputs as [{Player.name: feature dict}] (status checked)."""
    out = []
    for i in range(len(recs)):
        for r in recs[i]:
            _check(r)
        out.append({p.name: dict(zip(SNAPSHOT_FEATURE_COLUMNS, feats[i, j].tolist())) for j, p in enumerate(_PLAYERS)})
    return out


def coerce_feature_dict(features: Mapping[str, Any]) -> Dict[str, float]:
    """The canonical row of a feature mapping: every column, as a float, a missing one 0.0."""
    return {c: float(features.get(c, 0.0)) for c in SNAPSHOT_FEATURE_COLUMNS}
