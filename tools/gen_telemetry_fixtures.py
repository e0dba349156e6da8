#!/usr/bin/env python3
"""Generate tests/golden/telemetry.json from the reference implementation.

Like tools/gen_fixtures.py this imports a read-only checkout of the reference
($BLOKUS_REFERENCE) and records its behaviour; only the JSON it writes is committed.  Run
it from a scratch directory so nothing is written into the reference tree (about 4
CPU-minutes, spread over a process pool)::

    cd /tmp && BLOKUS_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python <repo>/tools/gen_telemetry_fixtures.py

For every record of tests/golden/positions.json (rebuilt with
generate_random_valid_state(num_moves, seed)) and a few late-game positions of its own
(stored with their place_piece log) it records, per player:

* the reference's collect_all_player_metrics dict for fast_mode=True (k = 3), and for
  every 8th position also fast_mode=False (k = 8), as value lists in METRIC_KEYS order;
* the integers behind it, from the reference's own functions: placements per piece and
  the busiest anchor, frontier size / clusters / quadrants, centre distance, the dead
  space split, and the stability run -- the indices the seeded shuffle picks in each
  opponent's list, the player's move count after each picked move (before sorting) and
  the number of 32-bit generator outputs the shuffles consumed (a counting
  random.Random stands in for engine.telemetry's).

Four delta cases hold the before / after dicts of consecutive moves of a reference
BlokusGame and its compute_move_telemetry_delta output.  The coverage the GPU tests rely
on is asserted before anything is written.
"""
from __future__ import annotations

import json
import os
import random
import sys
import types
from multiprocessing import Pool

REF = os.environ.get("BLOKUS_REFERENCE", "")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
OUT = os.path.join(GOLDEN, "telemetry.json")

# late-game positions of this fixture's own: a stuck player beside players that can move,
# and opponents with one or two moves (fewer than k)
EXTRA_SPECS = [(46, 101), (48, 109)]
K8_EVERY = 8
DELTA_SPEC = (28, 33)  # the delta cases: four consecutive moves from this position
MT_OUTPUTS = 16384
SHUFFLE_MAX = 2048
SIZE_LIMIT = 200 * 1024


def _build(num_moves, seed):
    """generate_random_valid_state with the place_piece log."""
    import engine.board as eb
    from tests.utils_game_states import generate_random_valid_state
    log = []
    orig = eb.Board.place_piece

    def logged(self, positions, player, piece_id, validate=True):
        ok = orig(self, positions, player, piece_id, validate)
        if ok:
            log.append([player.value, piece_id, [[p.row, p.col] for p in positions]])
        return ok

    eb.Board.place_piece = logged
    try:
        board, _ = generate_random_valid_state(num_moves, seed)
    finally:
        eb.Board.place_piece = orig
    return board, log


class _CountingRandom(random.Random):
    """random.Random that counts the 32-bit outputs its shuffles consume."""
    made = []

    def __init__(self, *a):
        super().__init__(*a)
        self.draws = 0
        _CountingRandom.made.append(self)

    def getrandbits(self, k):
        self.draws += (k + 31) // 32
        return super().getrandbits(k)


def _mode(board, mg, fast_mode):
    """The reference's dict and the integers behind it for one board and mode."""
    import engine.telemetry as T
    from engine.advanced_metrics import (compute_center_proximity, compute_dead_space_split,
                                         compute_frontier_spread)
    from engine.board import Player
    k = T.TelemetryConfig.MOBILITY_SAMPLES_K if fast_mode else 8
    _CountingRandom.made = []
    real = T.random
    T.random = types.SimpleNamespace(Random=_CountingRandom)
    try:
        metrics = T.collect_all_player_metrics(board, mg, fast_mode)
    finally:
        T.random = real
    assert all(sorted(m) == sorted(METRIC_KEYS) for m in metrics.values())  # every key is recorded
    draws = [r.draws for r in _CountingRandom.made]
    assert len(draws) == 4
    lists = {p: mg.get_legal_moves(board, p) for p in Player}
    ints = []
    for i, p in enumerate(Player):
        moves = lists[p]
        per_piece = [0] * 21
        anchors = {}
        for m in moves:
            per_piece[m.piece_id - 1] += 1
            anchors[(m.anchor_row, m.anchor_col)] = anchors.get((m.anchor_row, m.anchor_col), 0) + 1
        comps, quads = compute_frontier_spread(board, p)
        ds_self, ds_opp = compute_dead_space_split(board, p)
        picks, after = [], []
        if moves:
            rng = random.Random(T.TelemetryConfig.DETERMINISM_SEED)
            for q in Player:
                if q == p or not lists[q]:
                    continue
                order = list(range(len(lists[q])))
                rng.shuffle(order)
                for j in order[:k]:
                    mv = lists[q][j]
                    trial = board.copy()
                    trial.place_piece(mv.get_positions(mg.piece_orientations_cache[mv.piece_id]), q, mv.piece_id)
                    picks.append(j)
                    after.append(len(mg.get_legal_moves(trial, p)))
        # the replay above is the reference's run: its sorted summary must come out the same
        if after:
            srt = sorted(float(x) for x in after)
            assert metrics[p.name]["mobilityNextMean"] == sum(srt) / len(srt)
            assert metrics[p.name]["mobilityNextMin"] == srt[0]
            assert metrics[p.name]["mobilityNextP10"] == srt[max(0, int(0.10 * len(srt)) - 1)]
        assert metrics[p.name]["mobility"] == float(len(moves))
        ints.append({"mobility": len(moves), "piece_count": per_piece,
                     "anchor_max": max(anchors.values()) if anchors else 0,
                     "frontier_size": len(board.get_frontier(p)), "frontier_components": comps,
                     "quadrants": quads, "center_dist": compute_center_proximity(board, p),
                     "dead_self": int(ds_self), "dead_opp": int(ds_opp), "sample_index": picks,
                     "sample_mobility": after, "rng_draws": draws[i]})
    return {"k": k, "metrics": {name: [m[key] for key in METRIC_KEYS] for name, m in metrics.items()},
            "ints": ints}


METRIC_KEYS = [
    "frontierSize", "effectiveFrontier", "frontierComponentCount", "frontierQuadrantCoverage", "centerControl",
    "centerControlWeighted", "pieceLockRisk", "remainingArea", "mobility", "mobilityWeighted", "mobilityEntropy",
    "pieceTop1Share", "anchorTop1Share", "mobilityNextMean", "mobilityNextP10", "mobilityNextMin",
    "mobilityDropRisk", "lockedArea", "criticalPiecesCount", "bottleneckScore", "largestRemainingPiece",
    "unloadPotential", "deadSpaceNearSelf", "deadSpaceNearOpponents", "deadSpace",
]


def gen_position(job):
    sys.path.insert(0, REF)
    from engine.advanced_metrics import compute_dead_zones
    from engine.board import Player
    from engine.move_generator import LegalMoveGenerator
    index, num_moves, seed, want_k8, expect_bits = job
    board, log = _build(num_moves, seed)
    if expect_bits is not None:
        assert [hex(board.player_bits[p]) for p in Player] == expect_bits, (num_moves, seed)
    mg = LegalMoveGenerator()
    rec = {"index": index, "num_moves": num_moves, "seed": seed, "fast": _mode(board, mg, True)}
    assert sorted(rec["fast"]["metrics"]) == sorted(p.name for p in Player)
    if want_k8:
        rec["k8"] = _mode(board, mg, False)
    if index is None:  # a position of this fixture's own: everything a test needs to rebuild it
        rec["log"] = log
        rec["state"] = {"current_player": board.current_player.value,
                        "used": [sorted(board.player_pieces_used[p]) for p in Player]}
    dead_cells = sum(1 for row in compute_dead_zones(board) for x in row if x)
    edge = lambda v: v < 3 or v > 16  # noqa: E731
    rec["_cover"] = {
        "corner_key": any(edge(r) and edge(c) for p in Player for r, c in board.get_frontier(p)),
        # a pocket two players both count as theirs borders self and an opponent for each
        "shared_pocket": sum(i["dead_self"] for i in rec["fast"]["ints"]) > dead_cells,
    }
    return rec


def gen_deltas(_):
    sys.path.insert(0, REF)
    from engine.game import BlokusGame
    board, _log = _build(*DELTA_SPEC)
    game = BlokusGame()
    game.board = board
    rnd = random.Random(7)
    cases = []
    while len(cases) < 4:
        moves = game.get_legal_moves()
        if not moves:
            game.board._update_current_player()
            continue
        assert game.make_move(rnd.choice(moves))
        tel = dict(game.game_history[-1]["telemetry"])
        before = {e["playerId"]: e["metrics"] for e in tel.pop("before")}
        after = {e["playerId"]: e["metrics"] for e in tel.pop("after")}
        cases.append({"ply": tel["ply"], "moverId": tel["moverId"], "moveId": tel["moveId"],
                      "before": before, "after": after, "expected": tel})
    return cases


def main():
    if not os.path.isdir(os.path.join(REF, "engine")):
        sys.exit("set BLOKUS_REFERENCE to a checkout of the reference")
    positions = json.load(open(os.path.join(GOLDEN, "positions.json")))
    jobs = [(i, r["num_moves"], r["seed"], i % K8_EVERY == 0, r["state"]["player_bits"])
            for i, r in enumerate(positions)]
    jobs += [(None, m, s, True, None) for m, s in EXTRA_SPECS]
    with Pool(min(16, os.cpu_count() or 4)) as pool:
        delta_job = pool.map_async(gen_deltas, [0])
        recs = pool.map(gen_position, jobs, chunksize=1)
        deltas = delta_job.get()[0]

    # ---- coverage the GPU tests rely on
    modes = [m for r in recs for m in (r["fast"], r.get("k8")) if m]
    players = [(m, i) for m in modes for i in range(4)]
    mob = lambda m, i: m["ints"][i]["mobility"]  # noqa: E731
    cover = {
        "empty_board": any(r["num_moves"] == 0 for r in recs),
        "stuck_player": any(mob(m, i) == 0 for m, i in players),
        "skipped_opponent": any(mob(m, i) > 0 and any(mob(m, q) == 0 for q in range(4) if q != i)
                                for m, i in players),
        "short_list": any(mob(m, i) > 0 and any(1 <= mob(m, q) < m["k"] for q in range(4) if q != i)
                          for m, i in players),
        "five_components": any(m["ints"][i]["frontier_components"] >= 5 for m, i in players),
        "corner_key": any(r["_cover"]["corner_key"] for r in recs),
        "shared_pocket": any(r["_cover"]["shared_pocket"] for r in recs),
        "both_dead_kinds": any(m["ints"][i]["dead_self"] > 0 and m["ints"][i]["dead_opp"] > 0 for m, i in players),
    }
    max_draws = max(m["ints"][i]["rng_draws"] for m, i in players)
    max_list = max(mob(m, i) for m, i in players)
    missing = [k for k, v in cover.items() if not v]
    assert not missing, f"coverage missing: {missing}"
    # no fixture case may be excused through a status bit
    assert max_draws < MT_OUTPUTS and max_list < SHUFFLE_MAX, (max_draws, max_list)
    for r in recs:
        del r["_cover"]
    doc = {"metric_keys": METRIC_KEYS, "positions": recs, "deltas": deltas,
           "coverage": dict(cover, max_draws=max_draws, max_list=max_list)}
    text = json.dumps(doc, separators=(",", ":"))
    assert len(text) < SIZE_LIMIT, len(text)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(f"wrote {OUT}: {len(text)} bytes, {len(recs)} positions, max draws {max_draws}, max list {max_list}")


if __name__ == "__main__":
    main()
