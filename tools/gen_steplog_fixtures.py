#!/usr/bin/env python3
"""Generate tests/golden/steplog_game.json and tests/golden/steplog_steps.json from the
reference implementation.

Like tools/gen_telemetry_fixtures.py this imports a read-only checkout of the reference
($BLOKUS_REFERENCE) and records its behaviour; only the JSON it writes is committed.  Run
it from a scratch directory so nothing is written into the reference tree (CPU only, about
a minute over a process pool; the in-tree library must be built, its host-side table code
packs the frontier tables)::

    cd /tmp && BLOKUS_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python <repo>/tools/gen_steplog_fixtures.py

steplog_game.json: the reference StrategyLogger's lines for the sample game of the
reference's scripts/generate_analytics_data.py (four RandomAgent(seed=p.value),
BlokusGame(enable_telemetry=False)) minus ``timestamp``, its results.jsonl line, and per
step the integers of bk_step_rec.

steplog_steps.json: one step per record of tests/golden/positions.json (rebuilt with
generate_random_valid_state(num_moves, seed); the current player advances past stuck
players; the move is random.Random(seed).choice of the mover's legal list) and extras of
this fixture's own (EXTRA_SPECS: builder, num_moves, seed, move seed; a position of
frontier-greedy play, _build_greedy, and random positions with another move seed).  Each case holds

* the packed bk_state / bk_fset of the board before (a Board.copy(), as the logger's caller
  passes) and after the move (zlib + base64 of the records; the tables come from replaying
  the place_piece log through this package's Board, and their key order is checked against
  the reference's own set iteration),
* the step (mover 0..3, piece_id, orientation, anchor_row, anchor_col),
* the integers of bk_step_rec from the reference's own lists, sets and metric functions,
* the 28 metrics as the reference's logger merges them.

The coverage the tests rely on is asserted before anything is written.
"""
from __future__ import annotations

import base64
import json
import os
import random
import sys
import zlib
from multiprocessing import Pool

REF = os.environ.get("BLOKUS_REFERENCE", "")
REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLDEN = os.path.join(REPO, "tests", "golden")
OUT_GAME = os.path.join(GOLDEN, "steplog_game.json")
OUT_STEPS = os.path.join(GOLDEN, "steplog_steps.json")
SIZE_LIMIT = 200 * 1024

# steps of this fixture's own (builder, num_moves, seed, move seed).  "greedy" (_build_greedy):
# every player takes the placement that leaves it the most frontier cells, which grows a
# frontier table to 256 slots (random play stays at 128 or fewer).  "random" (_build, as the
# positions.json records) with a move seed of its own: a tie for the greatest loss
EXTRA_SPECS = [("greedy", 44, 10, 10), ("random", 28, 34, 100)]
GREEDY_CANDIDATES = 24

REC_FIELDS = ("moves_before", "moves_after", "frontier_before", "frontier_after", "area_before", "area_after",
              "perimeter_before", "perimeter_after", "bbox_area_after", "center_dist_sum", "center_gain",
              "placed_cells", "dist_to_opp_min", "status")


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


def _build_greedy(num_moves, seed):
    """A position after num_moves placements of frontier-greedy players, with the place_piece
    log: each mover takes, of GREEDY_CANDIDATES legal moves drawn by random.Random(seed), the
    first that leaves it the largest frontier."""
    from engine.board import Board
    from engine.move_generator import LegalMoveGenerator
    mg, rnd, board, log, stuck = LegalMoveGenerator(), random.Random(seed), Board(), [], 0
    while len(log) < num_moves and stuck < 4:
        player = board.current_player
        legal = mg.get_legal_moves(board, player)
        if not legal:
            board._update_current_player()
            stuck += 1
            continue
        stuck, best, best_size = 0, None, -1
        for mv in rnd.sample(legal, min(len(legal), GREEDY_CANDIDATES)):
            trial = board.copy()
            positions = mv.get_positions(mg.piece_orientations_cache[mv.piece_id])
            trial.place_piece(positions, player, mv.piece_id)
            if len(trial.get_frontier(player)) > best_size:
                best, best_size = (mv, positions), len(trial.get_frontier(player))
        assert board.place_piece(best[1], player, best[0].piece_id)
        log.append([player.value, best[0].piece_id, [[q.row, q.col] for q in best[1]]])
    assert len(log) == num_moves
    return board, log


def _reference_step(state, move, next_state, player_id, mg):
    """The logger's merged metric dict, and the integers of bk_step_rec behind it, from the
    reference's own functions."""
    import numpy as np
    from analytics.metrics import (CENTER_COORD, MetricInput, compute_blocking_metrics, compute_center_metrics,
                                   compute_corner_metrics, compute_mobility_metrics, compute_piece_metrics,
                                   compute_proximity_metrics, compute_territory_metrics, mdist)
    from analytics.metrics.mobility import get_mobility_counts
    from engine.board import Player
    placed = [(p.row, p.col) for p in move.get_positions(mg.piece_orientations_cache[move.piece_id])]
    opponents = [p.value for p in Player if p.value != player_id]
    inp = MetricInput(state=state, move=move, next_state=next_state, player_id=player_id, opponents=opponents,
                      placed_squares=placed, precomputed_values={})
    before, after = get_mobility_counts(inp)
    inp.precomputed_values["mobility_counts_before"] = before
    inp.precomputed_values["mobility_counts_after"] = after
    metrics = {}
    for fn in (compute_center_metrics, compute_territory_metrics, compute_mobility_metrics, compute_blocking_metrics,
               compute_corner_metrics, compute_proximity_metrics, compute_piece_metrics):
        metrics.update(fn(inp))
    metrics = json.loads(json.dumps(metrics, default=float))  # (numpy floats as JSON writes them)
    assert len(metrics) == 28
    mask_after = next_state.grid == player_id
    rows, cols = np.where(mask_after)
    bbox = int((rows.max() - rows.min() + 1) * (cols.max() - cols.min() + 1))
    area_before = int(np.sum(state.grid == player_id))
    area_after = int(np.sum(mask_after))
    assert area_after - area_before == metrics["area_gain"] and area_after / bbox == metrics["bbox_fill_after"]
    dsum = sum(mdist(sq, CENTER_COORD) for sq in placed)
    assert dsum == int(dsum) and dsum / len(placed) == metrics["center_distance"]
    ints = {
        "moves_before": [before[p.value] for p in Player], "moves_after": [after[p.value] for p in Player],
        "frontier_before": [len(state.get_frontier(p)) for p in Player],
        "frontier_after": [len(next_state.get_frontier(p)) for p in Player],
        "area_before": area_before, "area_after": area_after,
        "perimeter_before": metrics["perimeter_after"] - metrics["delta_perimeter"],
        "perimeter_after": metrics["perimeter_after"], "bbox_area_after": bbox, "center_dist_sum": int(dsum),
        "center_gain": metrics["center_gain"], "placed_cells": len(placed),
        "dist_to_opp_min": int(metrics["dist_to_opp_min"]), "status": 0,
    }
    assert metrics["dist_to_opp_min"] == ints["dist_to_opp_min"] and list(ints) == list(REC_FIELDS)
    return metrics, ints, placed, opponents


def _nearest(state, placed, opponents, dmin):
    """Where the nearest opponent cells lie relative to the placed cell they are nearest to."""
    import numpy as np
    opp = [tuple(x) for x in np.argwhere(np.isin(state.grid, opponents))]
    pairs = [(r, c, orr, oc) for r, c in placed for orr, oc in opp if abs(r - orr) + abs(c - oc) == dmin]
    return {"same_row": any(r == orr for r, c, orr, oc in pairs), "same_col": any(c == oc for r, c, orr, oc in pairs),
            "far_side_only": bool(pairs) and all(oc > c for r, c, orr, oc in pairs)}


def _cover(state, metrics, ints, placed, opponents, player_id):
    losses = [max(0, ints["moves_before"][o - 1] - ints["moves_after"][o - 1]) for o in opponents]
    d = ints["dist_to_opp_min"]
    near = _nearest(state, placed, opponents, d) if d < 40 else {"same_row": False, "same_col": False,
                                                                 "far_side_only": False}
    return {
        "first_move": ints["area_before"] == 0 and ints["perimeter_before"] == 0 and d == 40,
        "row_0": any(r == 0 for r, _ in placed), "row_19": any(r == 19 for r, _ in placed),
        "col_0": any(c == 0 for _, c in placed), "col_19": any(c == 19 for _, c in placed),
        "monomino": len(placed) == 1, "five_cells": len(placed) == 5,
        "dist_1": d == 1, "dist_3": d == 3, "dist_4": d == 4, "dist_10_plus": 10 <= d < 40,
        "nearest_same_row": near["same_row"], "nearest_same_col": near["same_col"],
        "nearest_far_side_only": near["far_side_only"],
        "mover_stuck_after": ints["moves_after"][player_id - 1] == 0,
        "opponent_stuck_both": any(ints["moves_before"][o - 1] == 0 and ints["moves_after"][o - 1] == 0
                                   for o in opponents),
        "blocking_not_first": metrics["blocking"] > 0 and metrics["blocking_target_id"] != opponents[0],
        "blocking_tie": max(losses) > 0 and losses.count(max(losses)) > 1,
        "center_gain": ints["center_gain"] > 0,
        "ratio_above_1": metrics["mobility_me_ratio"] > 1.0, "ratio_below_1": 0.0 < metrics["mobility_me_ratio"] < 1.0,
    }


def _pack_pair(board_before, board_after, log, step_cells, player_id, piece_id):
    """(state, sets) of the before board (a copy) and the after board, through this package's Board."""
    sys.path.insert(0, REPO)
    import numpy as np

    from reinforcementlearning_blokus_amd.engine import board as gb
    b = gb.Board()
    for player_value, pid, cells in log:
        b.current_player = gb.Player(player_value)
        b.place_piece([gb.Position(r, c) for r, c in cells], gb.Player(player_value), pid, validate=False)
    b.current_player = gb.Player(player_id)
    before = b.copy()
    assert b.place_piece([gb.Position(r, c) for r, c in step_cells], gb.Player(player_id), piece_id)
    enc = lambda a: base64.b64encode(zlib.compress(np.ascontiguousarray(a).tobytes(), 9)).decode()  # noqa: E731
    out, tables = [], {"dummy_slot": False, "mask_255": False}
    for mine, ref in ((before, board_before), (b, board_after)):
        state, sets = gb.pack_state(mine), gb.pack_fsets([mine])
        for i, p in enumerate(type(ref.current_player)):
            assert int(mine.player_bits[gb.Player(p.value)]) == int(ref.player_bits[p])
            mask = int(sets[0]["mask"][i])
            keys = [int(k) for k in sets[0]["key"][i, : mask + 1]]
            assert [k for k in keys if k >= 0] == [r * 20 + c for r, c in ref.get_frontier(p)], "table layout differs"
            tables["dummy_slot"] |= -2 in keys
            tables["mask_255"] |= mask == 255
        assert int(state[0]["move_count"]) == ref.move_count
        out.append({"state": enc(state), "sets": enc(sets)})
    return out[0], out[1], tables


def gen_case(job):
    sys.path.insert(0, REF)
    from engine.board import Player
    from engine.move_generator import LegalMoveGenerator
    index, num_moves, seed, move_seed, expect_bits = job
    board, log = _build_greedy(num_moves, seed) if index == "greedy" else _build(num_moves, seed)
    if expect_bits is not None:
        assert [hex(board.player_bits[p]) for p in Player] == expect_bits, (num_moves, seed)
    mg = LegalMoveGenerator()
    legal = []
    for _ in range(4):  # past stuck players, as generate_random_valid_state advances
        legal = mg.get_legal_moves(board, board.current_player)
        if legal:
            break
        board._update_current_player()
    if not legal:
        return None  # the position is terminal: no step
    player = board.current_player
    move = random.Random(move_seed).choice(legal)
    state = board.copy()
    positions = move.get_positions(mg.piece_orientations_cache[move.piece_id])
    assert board.place_piece(positions, player, move.piece_id)
    metrics, ints, placed, opponents = _reference_step(state, move, board, player.value, mg)
    before, after, tables = _pack_pair(state, board, log, placed, player.value, move.piece_id)
    cover = dict(_cover(state, metrics, ints, placed, opponents, player.value), **tables)
    index = index if isinstance(index, int) else None  # (None: a step of this fixture's own)
    return {"index": index, "num_moves": num_moves, "seed": seed, "move_seed": move_seed, "player_id": player.value,
            "step": [player.value - 1, move.piece_id, move.orientation, move.anchor_row, move.anchor_col],
            "before": before, "after": after, "ints": ints, "metrics": metrics, "_cover": cover}


def gen_game(_):
    """The reference logger's files for the sample game, and the integers behind each line."""
    sys.path.insert(0, REF)
    import tempfile

    import analytics.logging.logger as L
    from agents.random_agent import RandomAgent
    from engine.board import Player
    from engine.game import BlokusGame
    records, covers = [], []
    orig = L.StrategyLogger.on_step

    def on_step(self, game_id, turn_index, player_id, state, move, next_state):
        metrics, ints, placed, opponents = _reference_step(state, move, next_state, player_id, self.move_generator)
        records.append(ints)
        covers.append(_cover(state, metrics, ints, placed, opponents, player_id))
        orig(self, game_id, turn_index, player_id, state, move, next_state)

    L.StrategyLogger.on_step = on_step
    with tempfile.TemporaryDirectory() as tmp:
        logger = L.StrategyLogger(log_dir=tmp)
        agents = {p: RandomAgent(seed=p.value) for p in Player}
        game = BlokusGame(enable_telemetry=False)
        logger.on_reset("game_001", 42, {p.value: f"RandomAgent_{p.name}" for p in Player}, {})
        turn_index = 0
        while not game.is_game_over():  # the loop of scripts/generate_analytics_data.py
            player = game.get_current_player()
            before = game.get_board_copy()
            legal = game.get_legal_moves(player)
            if not legal:
                game.board._update_current_player()
                game._check_game_over()
                continue
            move = agents[player].select_action(game.board, player, legal)
            assert move is not None and game.make_move(move, player)
            logger.on_step("game_001", turn_index, player.value, before, move, game.board)
            turn_index += 1
        res = game.get_game_result()
        logger.on_game_end("game_001", res.scores, res.winner_ids[0] if not res.is_tie else None, turn_index)
        lines = [json.loads(x) for x in open(logger.steps_path)]
        results = [json.loads(x) for x in open(logger.results_path)]
    assert len(results) == 1 and len(lines) == len(records) == turn_index
    keys = list(lines[0])
    for ln, ints in zip(lines, records):
        assert list(ln) == keys and len(ln["metrics"]) == 28
        assert ln["legal_moves_before"] == ints["moves_before"][ln["player_id"] - 1]
        del ln["timestamp"]
    del results[0]["timestamp"]
    return {"game_id": "game_001", "seed": 42, "lines": lines, "result": results[0], "records": records}, covers


def main():
    if not os.path.isdir(os.path.join(REF, "engine")):
        sys.exit("set BLOKUS_REFERENCE to a checkout of the reference")
    positions = json.load(open(os.path.join(GOLDEN, "positions.json")))
    jobs = [(i, r["num_moves"], r["seed"], r["seed"], r["state"]["player_bits"]) for i, r in enumerate(positions)]
    jobs += [(kind, m, s, ms, None) for kind, m, s, ms in EXTRA_SPECS]
    with Pool(min(16, os.cpu_count() or 4)) as pool:
        game_job = pool.map_async(gen_game, [0])
        cases = [c for c in pool.map(gen_case, jobs, chunksize=1) if c is not None]
        game, game_covers = game_job.get()[0]

    # ---- coverage the tests rely on.  Each file stores the properties ITS OWN steps show, and
    # the step cases, which go through the kernel record by record, must show every one
    covers = [c["_cover"] for c in cases]
    cover = {k: any(c[k] for c in covers) for k in covers[0]}
    game_cover = {k: any(c[k] for c in game_covers) for k in game_covers[0]}
    missing = [k for k, v in cover.items() if not v]
    assert not missing, f"coverage missing from the step cases: {missing}; the game shows {game_cover}"
    game["coverage"] = game_cover
    # no case may be excused through a status bit: every recorded status is 0
    assert all(c["ints"]["status"] == 0 for c in cases) and all(r["status"] == 0 for r in game["records"])
    for c in cases:
        del c["_cover"]
    for path, doc in ((OUT_STEPS, {"rec_fields": list(REC_FIELDS), "cases": cases, "coverage": cover}),
                      (OUT_GAME, game)):
        text = json.dumps(doc, separators=(",", ":"))
        assert len(text) < SIZE_LIMIT, (path, len(text))
        with open(path, "w") as f:
            f.write(text + "\n")
        print(f"wrote {path}: {len(text)} bytes")
    print(f"{len(cases)} step cases, {len(game['lines'])} game steps")


if __name__ == "__main__":
    sys.path.insert(0, REF)
    main()
