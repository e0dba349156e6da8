"""Per-move telemetry on the GPU (reference: engine/telemetry.py, engine/metrics_config.py).

The reference computes, before and after every move, some thirty metrics per player from
about 44 legal-move generations and a handful of board scans.  Here one bk_telemetry
launch (gpu.BlokusGPU.telemetry) returns the integers behind all of them for any number
of boards -- move counts per piece, the busiest anchor, frontier clusters, dead space, the
stability samples of the seeded shuffle, and the one float that is summed on the device
(effectiveFrontier, bit-exact) -- and ``metrics_from_record`` turns a record into the
reference's dict with ``math`` arithmetic in the reference's order, so every float
equals CPython's.  There is no CPU implementation of the board work behind this module.
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Sequence

from .board import Board, Player, pack_fsets, pack_states
from .mobility_metrics import mobility_from_counts, piece_tables

_PLAYERS = list(Player)


class TelemetryConfig:
    """Knobs and weights of the telemetry (engine/metrics_config.py)."""
    MOBILITY_SAMPLES_K = 3    # opponent moves sampled per opponent in fast mode (8 otherwise)
    PIECE_SUBSET_N = 5
    ANCHOR_RADIUS = 3         # the effective-frontier box is (2 R + 1) squared
    ENABLE_FULL_ENUM = False
    DETERMINISM_SEED = 42     # the stability shuffle's random.Random seed (fixed in the library)

    # +1: more is better for the player, -1: less is better (advantage deltas)
    METRIC_POLARITY: Dict[str, int] = {
        "frontierSize": 1, "effectiveFrontier": 1, "frontierComponentCount": 1, "frontierQuadrantCoverage": 1,
        "mobility": 1, "mobilityWeighted": 1, "mobilityEntropy": 1, "pieceTop1Share": -1, "anchorTop1Share": -1,
        "mobilityNextMean": 1, "mobilityNextP10": 1, "mobilityNextMin": 1, "mobilityDropRisk": -1,
        "centerControl": 1, "centerControlWeighted": 1,
        "deadSpaceNearOpponents": 1, "deadSpaceNearSelf": -1,
        "lockedArea": -1, "criticalPiecesCount": -1, "bottleneckScore": 1, "remainingArea": -1,
        "largestRemainingPiece": -1, "unloadPotential": 1,
        "deadSpace": 1, "pieceLockRisk": -1,
    }

    WIN_PROXY_WEIGHTS: Dict[str, float] = {
        "remainingAreaAdv": 2.0, "effectiveFrontierAdv": 1.5, "mobilityNextP10Adv": 1.5, "lockedAreaAdv": 1.0,
        "centerControlWeightedAdv": 0.5,
    }


def _stability(mobility: int, samples: Sequence[float]) -> Dict[str, float]:
    """mean / 10th percentile / min of the player's move count after each sampled opponent
    move, and the drop from the current count to that percentile."""
    if mobility == 0:
        return {"mobilityNextMean": 0.0, "mobilityNextP10": 0.0, "mobilityNextMin": 0.0, "mobilityDropRisk": 0.0}
    if not samples:
        cur = float(mobility)
        return {"mobilityNextMean": cur, "mobilityNextP10": cur, "mobilityNextMin": cur, "mobilityDropRisk": 0.0}
    ordered = sorted(samples)
    n = len(ordered)
    p10 = ordered[max(0, int(0.10 * n) - 1)]
    return {"mobilityNextMean": sum(ordered) / n, "mobilityNextP10": p10, "mobilityNextMin": ordered[0],
            "mobilityDropRisk": max(0.0, mobility - p10)}


def metrics_from_record(rec, pieces_used: Iterable[int], with_moves: bool = True) -> Dict[str, float]:
    """One player's bk_player_metrics record (a numpy record or any mapping with its field
    names) as the reference's metric dict (compute_player_metrics plus the dead-space keys
    collect_all_player_metrics adds).  Host arithmetic only.  with_moves=False gives the
    reference's ``move_generator is None`` fallbacks for the move-based keys."""
    used = set(int(x) for x in pieces_used)
    _, sizes = piece_tables()
    held = [pid for pid in range(1, 22) if pid not in used]
    remaining_area = sum(sizes[pid] for pid in held)
    phase = max(0.0, min(1.0, 1.0 - (remaining_area / 89.0)))
    center_raw = 9.0 - int(rec["center_dist"])
    frontier_size = int(rec["frontier_size"])
    out: Dict[str, float] = {
        "frontierSize": float(frontier_size),
        "effectiveFrontier": float(rec["effective_frontier"]),
        "frontierComponentCount": float(int(rec["frontier_components"])),
        "frontierQuadrantCoverage": float(int(rec["quadrants"])),
        "centerControl": float(center_raw),
        "centerControlWeighted": float(center_raw * phase),
        "pieceLockRisk": 0.0,
        "remainingArea": float(remaining_area),
    }
    if with_moves:
        if int(rec["status"]):
            raise RuntimeError(f"bk_telemetry: stability samples invalid (status {int(rec['status'])})")
        mobility = int(rec["mobility"])
        counts = [int(c) for c in rec["piece_count"]]
        placements = {pid: counts[pid - 1] for pid in range(1, 22) if counts[pid - 1] > 0}
        mob = mobility_from_counts(placements, int(rec["anchor_max"]), used)
        out["mobility"] = float(mobility)
        out["mobilityWeighted"] = mob.totalCellWeighted
        out["mobilityEntropy"] = mob.mobilityEntropy
        out["pieceTop1Share"] = mob.pieceTop1Share
        out["anchorTop1Share"] = mob.anchorTop1Share
        n = int(rec["n_samples"])
        out.update(_stability(mobility, [float(int(x)) for x in list(rec["sample_mobility"])[:n]]))
        per_piece = {pid: placements.get(pid, 0) for pid in held}
        stuck = [pid for pid in held if per_piece[pid] == 0]
        out["pieceLockRisk"] = float(len(stuck))
        out["lockedArea"] = float(sum(sizes[pid] for pid in stuck))
        out["criticalPiecesCount"] = float(sum(1 for c in per_piece.values() if 0 < c <= 3))
        placed = [c for c in per_piece.values() if c > 0]
        out["bottleneckScore"] = float(min(placed)) if placed else 0.0
        out["largestRemainingPiece"] = float(max((sizes[pid] for pid in held), default=0))
        out["unloadPotential"] = float(sum(sizes[pid] for pid in held if per_piece[pid] > 0))
    else:
        guess = float(frontier_size * 2)
        out.update({"mobility": guess, "mobilityWeighted": guess * 3, "mobilityEntropy": 0.0, "pieceTop1Share": 0.0,
                    "anchorTop1Share": 0.0, "mobilityNextMean": guess, "mobilityNextP10": guess,
                    "mobilityNextMin": guess, "mobilityDropRisk": 0.0, "lockedArea": 0.0,
                    "criticalPiecesCount": 0.0, "bottleneckScore": 0.0, "largestRemainingPiece": 0.0,
                    "unloadPotential": 0.0})
    near_self, near_opp = float(int(rec["dead_self"])), float(int(rec["dead_opp"]))
    out["deadSpaceNearSelf"] = near_self
    out["deadSpaceNearOpponents"] = near_opp
    out["deadSpace"] = near_self + near_opp
    return out


def _engine(move_generator=None):
    if move_generator is not None and hasattr(move_generator, "_engine"):
        return move_generator._engine()
    from ..gpu import BlokusGPU
    return BlokusGPU.shared(getattr(move_generator, "device", 0))


def _records(boards: Sequence[Board], move_generator, fast_mode: bool):
    k = TelemetryConfig.MOBILITY_SAMPLES_K if fast_mode else 8
    return _engine(move_generator).telemetry(pack_states(boards), pack_fsets(boards), k_samples=k,
                                             stability=move_generator is not None)


def _board_metrics(board: Board, recs, with_moves: bool) -> Dict[str, Dict[str, float]]:
    return {p.name: metrics_from_record(recs[i], board.player_pieces_used[p], with_moves)
            for i, p in enumerate(_PLAYERS)}


_DEAD_KEYS = ("deadSpaceNearSelf", "deadSpaceNearOpponents", "deadSpace")


def compute_player_metrics(board: Board, player: Player, move_generator=None, fast_mode: bool = True) -> Dict[str, float]:
    """One player's metrics without the dead-space keys (which collect_all_player_metrics
    adds).  The launch computes all four players; the other three are dropped."""
    recs = _records([board], move_generator, fast_mode)[0]
    m = metrics_from_record(recs[player.value - 1], board.player_pieces_used[player], move_generator is not None)
    for k in _DEAD_KEYS:
        del m[k]
    return m


def collect_all_player_metrics(board: Board, move_generator=None, fast_mode: bool = True) -> Dict[str, Dict[str, float]]:
    """{Player.name: metrics} for the four players of one board: one GPU launch."""
    return _board_metrics(board, _records([board], move_generator, fast_mode)[0], move_generator is not None)


_DEFAULT_GENERATOR = object()


def collect_many(boards: Sequence[Board], fast_mode: bool = True, move_generator=_DEFAULT_GENERATOR) -> List[Dict[str, Dict[str, float]]]:
    """collect_all_player_metrics for every board in ONE launch (by default with the shared
    move generator's engine; move_generator=None gives the reference's fallbacks)."""
    if not boards:
        return []
    if move_generator is _DEFAULT_GENERATOR:
        from .move_generator import get_shared_generator
        move_generator = get_shared_generator()
    recs = _records(list(boards), move_generator, fast_mode)
    return [_board_metrics(b, recs[i], move_generator is not None) for i, b in enumerate(boards)]


def _advantage(snapshot: Dict[str, Dict[str, float]], player_id: str, key: str) -> float:
    """polarity * (the player's value - the mean of the others' values)."""
    if player_id not in snapshot or key not in snapshot[player_id]:
        return 0.0
    others = [snapshot[name][key] for name in snapshot if name != player_id and key in snapshot[name]]
    mean = sum(others) / len(others) if others else 0.0
    return float(TelemetryConfig.METRIC_POLARITY.get(key, 1) * (snapshot[player_id][key] - mean))


def _win_proxy(snapshot: Dict[str, Dict[str, float]], player_id: str) -> float:
    score = 0.0
    for name, weight in TelemetryConfig.WIN_PROXY_WEIGHTS.items():
        key = name.replace("Adv", "")
        if player_id in snapshot and key in snapshot[player_id]:
            score += _advantage(snapshot, player_id, key) * weight
    return score


def compute_move_telemetry_delta(ply: int, mover_id: str, move_id: str, before: Dict[str, Dict[str, float]],
                                 after: Dict[str, Dict[str, float]]) -> Dict[str, Any]:
    """What one move changed: the mover's own deltas, the opponents' (each and summed), the
    change of every advantage and of the weighted win proxy.  {} if the mover is missing
    from either snapshot."""
    if mover_id not in before or mover_id not in after:
        return {}
    delta_self = {k: v - before[mover_id].get(k, 0.0) for k, v in after[mover_id].items()}
    opp_total: Dict[str, float] = {}
    opp_each: Dict[str, Dict[str, float]] = {}
    for name, now in after.items():
        if name == mover_id:
            continue
        was = before.get(name, {})
        opp_each[name] = {}
        for k, v in now.items():
            d = v - was.get(k, 0.0)
            opp_each[name][k] = d
            opp_total[k] = opp_total.get(k, 0.0) + d
    adv: Dict[str, float] = {}
    for k in TelemetryConfig.METRIC_POLARITY:
        if k in after[mover_id]:
            was_adv = _advantage(before, mover_id, k)
            adv[k + "Adv"] = _advantage(after, mover_id, k) - was_adv
    proxy_before = _win_proxy(before, mover_id)
    adv["winProxy"] = _win_proxy(after, mover_id) - proxy_before
    return {"ply": ply, "moverId": mover_id, "moveId": move_id, "deltaSelf": delta_self,
            "deltaOppTotal": opp_total, "deltaOppByPlayer": opp_each, "deltaAdvantage": adv,
            "winProxyDelta": adv["winProxy"]}


def move_telemetry(ply: int, mover: Player, move, before: Optional[Dict], after: Dict) -> Optional[Dict[str, Any]]:
    """The ``telemetry`` block of a game-history entry (engine/game.py:127-146): the delta
    plus both snapshots as lists of {playerId, metrics}."""
    move_id = f"{move.piece_id}-{move.orientation}-{move.anchor_row}-{move.anchor_col}"
    payload = compute_move_telemetry_delta(ply=ply, mover_id=mover.name, move_id=move_id, before=before, after=after)
    if not payload:
        return None
    payload["before"] = [{"playerId": pid, "metrics": m} for pid, m in before.items()]
    payload["after"] = [{"playerId": pid, "metrics": m} for pid, m in after.items()]
    return payload
