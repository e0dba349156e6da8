"""Per-piece mobility metrics (reference: engine/mobility_metrics.py).

For every piece i the player still holds: P_i legal placements, O_i distinct orientations,
S_i cells; PN_i = P_i / O_i and MW_i = PN_i * S_i.  The sums, the entropy of the placement
distribution over pieces and the two concentration shares follow the reference's
arithmetic and accumulation order step for step, so the floats are CPython's.

``mobility_from_counts`` is the shared core: it needs only the per-piece counts and the
largest per-anchor count, which is what the GPU record (bk_player_metrics) carries.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Iterable, List

from .pieces import PieceGenerator


@dataclass
class PlayerMobilityMetrics:
    totalPlacements: int
    totalOrientationNormalized: float
    totalCellWeighted: float
    buckets: Dict[int, float]
    mobilityEntropy: float
    pieceTop1Share: float
    anchorTop1Share: float


_TABLES = None


def piece_tables():
    """({piece_id: O_i}, {piece_id: S_i}) for the 21 pieces."""
    global _TABLES
    if _TABLES is None:
        pieces = PieceGenerator.get_all_pieces()
        orients = {p.id: len(PieceGenerator.get_piece_rotations_and_reflections(p)) for p in pieces}
        sizes = {p.id: p.size for p in pieces}
        _TABLES = (orients, sizes)
    return _TABLES


def mobility_from_counts(placements: Dict[int, int], anchor_max: int, pieces_used: Iterable[int]) -> PlayerMobilityMetrics:
    """placements: {piece_id: P_i > 0} in the order the pieces first appear in the legal
    list (ascending piece id for the generator's lists); anchor_max: the largest number of
    legal moves sharing one (anchor_row, anchor_col), 0 for an empty list."""
    used = set(pieces_used)
    orients, sizes = piece_tables()
    total = 0
    total_norm = 0.0
    total_weighted = 0.0
    buckets: Dict[int, float] = {1: 0.0, 2: 0.0, 3: 0.0, 4: 0.0, 5: 0.0}
    top_piece = 0
    for pid in range(1, 22):
        if pid in used:
            continue
        count = placements.get(pid, 0)
        n_orient = orients.get(pid, 1)
        size = sizes.get(pid, 0)
        if size < 1 or size > 5:
            continue
        top_piece = max(top_piece, count)
        normalized = count / n_orient if n_orient > 0 else 0.0
        weighted = normalized * size
        total += count
        total_norm += normalized
        total_weighted += weighted
        buckets[size] = buckets.get(size, 0) + weighted

    entropy = 0.0
    if total > 0:
        acc = 0.0
        for pid, count in placements.items():
            if pid not in used and count > 0:
                share = count / total
                acc -= share * math.log(share)
        held = 21 - len(used)
        entropy = acc / math.log(held) if held > 1 else 0.0

    piece_share = top_piece / total if total > 0 else 0.0
    anchor_share = anchor_max / total if total > 0 and anchor_max > 0 else 0.0
    return PlayerMobilityMetrics(totalPlacements=total, totalOrientationNormalized=total_norm,
                                 totalCellWeighted=total_weighted, buckets=buckets, mobilityEntropy=entropy,
                                 pieceTop1Share=piece_share, anchorTop1Share=anchor_share)


def compute_player_mobility_metrics(legal_moves: List, pieces_used: List[int]) -> PlayerMobilityMetrics:
    """Mobility metrics of a legal-move list (objects with piece_id, anchor_row,
    anchor_col); pieces_used are excluded from every sum."""
    placements: Dict[int, int] = {}
    anchors: Dict[tuple, int] = {}
    for m in legal_moves:
        if 1 <= m.piece_id <= 21:
            placements[m.piece_id] = placements.get(m.piece_id, 0) + 1
        key = (m.anchor_row, m.anchor_col)
        anchors[key] = anchors.get(key, 0) + 1
    return mobility_from_counts(placements, max(anchors.values()) if anchors else 0, pieces_used)
