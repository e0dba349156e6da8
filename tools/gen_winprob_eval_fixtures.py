#!/usr/bin/env python3
"""Generate tests/golden/winprob_eval.json from the reference implementation.

Like tools/gen_winprob_fixtures.py this imports a read-only checkout of the reference
($BLOKUS_REFERENCE) and records its behaviour; only the JSON it writes is committed (nothing
pickled).  CPU only, about two minutes over a process pool; needs scikit-learn and joblib,
and the in-tree library built (its host-side table code packs the frontier tables)::

    cd /tmp && BLOKUS_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python <repo>/tools/gen_winprob_eval_fixtures.py

1. Two models are fitted on the reference's own arena snapshots (arena_runs/*/snapshots.csv):
   pairwise rows = differences of the 34 feature columns of two players of one game and
   checkpoint, label = "the first has the better final_rank", ties dropped;
   Pipeline([StandardScaler(), LogisticRegression(max_iter=2000)]).  The first model uses all
   34 columns, the second a permuted 20-column subset.
2. Each is written as the reference's joblib artifact into a temporary directory and loaded by
   the reference's LearnedWinProbabilityEvaluator.
3. For every position of winprob_features.json (the 56 golden positions and four late-game
   ones, rebuilt with gen_winprob_fixtures._build) the file holds the packed state and tables,
   the reference's four feature rows in the evaluator's own context (turn_index = move_count,
   max_turns = 2500), predict_player_win_probability of all four players, potential in both
   modes, pipeline.decision_function of the 12 ordered pairs, and the second model's
   probabilities.
4. Three short reference MCTSAgent searches from one late-game position (24 iterations,
   transposition table on, RandomAgent rollouts): leaf evaluation; leaf evaluation and
   progressive bias; potential shaping on 2-ply rollouts.
The models are stored in WinProbModel's JSON form.  The coverage the tests rely on is asserted
before anything is written.
"""
from __future__ import annotations

import csv
import glob
import json
import os
import sys
import tempfile
import time
from multiprocessing import Pool

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_winprob_fixtures as G  # noqa: E402  (_build, _pack, REF, EXTRA_SPECS)

REF, REPO, GOLDEN = G.REF, G.REPO, G.GOLDEN
OUT = os.path.join(GOLDEN, "winprob_eval.json")
MAX_TURNS = 2500
SUBSET_SEED, SUBSET_SIZE = 20260302, 20
SEARCH_ITERATIONS, SEARCH_MAX_LEGAL = 24, 12
SEARCH_ROLLOUT_SEED, SEARCH_ZOBRIST_SEED = 9001, 9002
SEARCHES = [
    {"name": "leaf", "options": {"leaf_evaluation_enabled": True}},
    {"name": "leaf_bias", "options": {"leaf_evaluation_enabled": True, "progressive_bias_enabled": True,
                                      "progressive_bias_weight": 0.25}},
    {"name": "shaping", "options": {"potential_shaping_enabled": True, "potential_shaping_gamma": 0.9,
                                    "potential_shaping_weight": 2.0, "max_rollout_moves": 2}},
]


def pairwise_rows(columns):
    """(X, y) over every ordered pair of players of one game and checkpoint."""
    import numpy as np
    groups = {}
    files = sorted(glob.glob(os.path.join(REF, "arena_runs", "*", "snapshots.csv")))
    n_rows = 0
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                n_rows += 1
                groups.setdefault((row["game_id"], row["checkpoint_index"]), []).append(
                    (int(row["final_rank"]), [float(row[c]) for c in columns]))
    X, y = [], []
    for members in groups.values():
        for i, (rank_i, f_i) in enumerate(members):
            for j, (rank_j, f_j) in enumerate(members):
                if i != j and rank_i != rank_j:
                    X.append([a - b for a, b in zip(f_i, f_j)])
                    y.append(1 if rank_i < rank_j else 0)
    return np.array(X, dtype=float), np.array(y), n_rows, len({g for g, _ in groups})


def fit(columns):
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    X, y, n_rows, n_games = pairwise_rows(columns)
    pipe = Pipeline([("scaler", StandardScaler()), ("model", LogisticRegression(max_iter=2000))])
    pipe.fit(X, y)
    return pipe, {"snapshot_rows": n_rows, "games": n_games, "pairs": int(len(y))}


_EVALS = {}


def _evaluator(path):
    sys.path.insert(0, REF)
    from mcts.learned_evaluator import LearnedWinProbabilityEvaluator
    if path not in _EVALS:
        _EVALS[path] = LearnedWinProbabilityEvaluator(path, max_turns=MAX_TURNS)
    return _EVALS[path]


def gen_position(job):
    sys.path.insert(0, REF)
    import numpy as np
    from analytics.winprob.features import SNAPSHOT_FEATURE_COLUMNS
    from engine.board import Player
    from engine.move_generator import LegalMoveGenerator
    index, num_moves, seed, art_full, art_subset = job
    board, log = G._build(num_moves, seed)
    ev, ev2 = _evaluator(art_full), _evaluator(art_subset)
    feats = ev._extract_features_for_all_players(board)   # the evaluator's own context
    for e in (ev, ev2):  # the reference's methods, over rows computed once for this board
        e._extract_features_for_all_players = lambda b, _f=feats: _f
    rows = [[feats[p.value][c] for c in SNAPSHOT_FEATURE_COLUMNS] for p in Player]
    prob = [ev.predict_player_win_probability(board, p) for p in Player]
    pots = {}
    for mode in ("prob", "logit"):
        ev.potential_mode = mode
        pots[mode] = [ev.potential(board, p) for p in Player]
    ev.potential_mode = "prob"
    pipe = ev.artifact["pipeline"]
    logit = []
    for p in Player:
        ts = []
        for q in Player:
            if q != p:
                x = np.array([[float(feats[p.value][c]) - float(feats[q.value][c]) for c in ev.feature_columns]],
                             dtype=float)
                ts.append(float(pipe.decision_function(x)[0]))
        logit.append(ts)
    prob_subset = [ev2.predict_player_win_probability(board, p) for p in Player]
    for e in (ev, ev2):
        del e._extract_features_for_all_players
    state, sets = G._pack(board, log)
    mg = LegalMoveGenerator()
    legal = {p.value: len(mg.get_legal_moves(board, p)) for p in Player}
    return {"index": index, "num_moves": num_moves, "seed": seed, "move_count": int(board.move_count),
            "state": state, "sets": sets, "rows": rows, "prob": prob, "potential_prob": pots["prob"],
            "potential_logit": pots["logit"], "logit": logit, "prob_subset": prob_subset,
            "_legal": legal, "_current": board.current_player.value}


def gen_search(job):
    sys.path.insert(0, REF)
    from agents.random_agent import RandomAgent
    from engine.board import Player
    from engine.move_generator import get_shared_generator
    from engine.pieces import ALL_PIECE_ORIENTATIONS
    from mcts.mcts_agent import MCTSAgent, MCTSNode
    spec, player_value, art_full, search = job
    board, log = G._build(*spec)
    player = Player(player_value)
    gid_of, g = {}, 0  # move ints as tools/gen_fixtures.py: g * 400 + row * 20 + col
    for pid in sorted(ALL_PIECE_ORIENTATIONS):
        for o in range(len(ALL_PIECE_ORIENTATIONS[pid])):
            gid_of[(pid, o)] = g
            g += 1

    def move_int(_, m):
        return gid_of[(m.piece_id, m.orientation)] * 400 + m.anchor_row * 20 + m.anchor_col

    legal = get_shared_generator().get_legal_moves(board, player)
    assert 2 <= len(legal) <= SEARCH_MAX_LEGAL
    agent = MCTSAgent(iterations=SEARCH_ITERATIONS, rollout_agent=RandomAgent(seed=SEARCH_ROLLOUT_SEED),
                      seed=SEARCH_ZOBRIST_SEED, use_transposition_table=True, learned_model_path=art_full,
                      **search["options"])
    t0 = time.time()
    root = MCTSNode(board, player)                      # select_action (:323-335) around the root
    agent._run_mcts_with_iterations(root)
    best = root.get_best_move()
    seconds = time.time() - t0
    st = agent.stats
    assert st["evaluator_errors"] == 0
    return {"name": search["name"], "options": search["options"], "iterations": SEARCH_ITERATIONS,
            "rollout_seed": SEARCH_ROLLOUT_SEED, "zobrist_seed": SEARCH_ZOBRIST_SEED, "n_legal": len(legal),
            "move": move_int(gid_of, best),
            "root_children": [[move_int(gid_of, ch.move), ch.visits, float(ch.prior_bias)] for ch in root.children],
            "iterations_run": st["iterations_run"], "transposition_hits": st["transposition_hits"],
            "rollout_rewards": [float(r) for r in st["rollout_rewards"]],
            "potential_shaping_terms": [float(r) for r in st["potential_shaping_terms"]],
            "leaf_eval_calls": st["leaf_eval_calls"], "progressive_bias_updates": st["progressive_bias_updates"],
            "reference_seconds": round(seconds, 3)}


def main():
    if not os.path.isdir(os.path.join(REF, "engine")):
        sys.exit("set BLOKUS_REFERENCE to a checkout of the reference")
    import joblib
    import numpy as np
    sys.path.insert(0, REPO)
    from reinforcementlearning_blokus_amd.analytics.winprob.features import SNAPSHOT_FEATURE_COLUMNS as COLUMNS
    from reinforcementlearning_blokus_amd.mcts.learned_evaluator import WinProbModel
    subset = [COLUMNS[i] for i in np.random.RandomState(SUBSET_SEED).permutation(len(COLUMNS))[:SUBSET_SIZE]]
    assert subset != sorted(subset, key=COLUMNS.index)
    pipe_full, train = fit(COLUMNS)
    pipe_subset, _ = fit(subset)
    coef = pipe_full.steps[-1][1].coef_[0]
    print(f"fitted on {train}: largest |coef| {abs(coef).max():.3f}, "
          f"{int((pipe_full.steps[0][1].var_ == 0).sum())} zero-variance columns")

    positions = json.load(open(os.path.join(GOLDEN, "positions.json")))
    specs = [(i, r["num_moves"], r["seed"]) for i, r in enumerate(positions)] + [(None, m, s) for m, s in G.EXTRA_SPECS]
    with tempfile.TemporaryDirectory() as tmp:
        art_full, art_subset = os.path.join(tmp, "full.pkl"), os.path.join(tmp, "subset.pkl")
        joblib.dump({"model_type": "pairwise_logreg", "feature_columns": list(COLUMNS), "pipeline": pipe_full}, art_full)
        joblib.dump({"model_type": "pairwise_logreg", "feature_columns": subset, "pipeline": pipe_subset}, art_subset)
        with Pool(min(16, os.cpu_count() or 4)) as pool:
            recs = pool.map(gen_position, [(i, m, s, art_full, art_subset) for i, m, s in specs], chunksize=1)
            # the search position: the latest position where a player has 2..12 legal moves and
            # the 2-ply rollouts of the shaping search are truncated at least four times
            cands = [(r["move_count"], n, pv) for n, r in enumerate(recs) if r["move_count"] >= 40
                     for pv in ([r["_current"]] + [v for v in (1, 2, 3, 4) if v != r["_current"]])
                     if 2 <= r["_legal"][pv] <= SEARCH_MAX_LEGAL]
            assert cands, "no late-game position with 2..12 legal moves"
            cands.sort(key=lambda c: (-c[0], c[1]))
            shaped = pool.map(gen_search, [((recs[n]["num_moves"], recs[n]["seed"]), pv, art_full, SEARCHES[2])
                                           for _, n, pv in cands], chunksize=1)
            pick = next(i for i, s in enumerate(shaped) if len(s["potential_shaping_terms"]) >= 4)
            _, at, player_value = cands[pick]
            spec = (recs[at]["num_moves"], recs[at]["seed"])
            searches = pool.map(gen_search, [(spec, player_value, art_full, s) for s in SEARCHES[:2]], chunksize=1)
            searches.append(shaped[pick])
    sys.path.insert(0, REF)
    board, log = G._build(*spec)
    search_doc = {"position": at, "num_moves": spec[0], "seed": spec[1], "player": player_value, "log": log,
                  "current_player": board.current_player.value, "searches": searches}

    # ---- coverage the tests rely on
    flat = [p for r in recs for p in r["prob"]]
    cover = {
        "ply_0_equal": any(r["move_count"] == 0 and len(set(r["prob"])) == 1 for r in recs),
        "stuck_player": any(row[COLUMNS.index("mobility_total_placements")] == 0.0 and r["move_count"] > 0
                            for r in recs for row in r["rows"]),
        "prob_below_0.05": min(flat) < 0.05,
        "prob_above_0.95": max(flat) > 0.95,
        "potential_unclipped": any(1e-6 < p < 1 - 1e-6 for p in flat),
        "leaf_calls": searches[0]["leaf_eval_calls"] > 0,
        "bias_updates": searches[1]["progressive_bias_updates"] > 0
        and any(ch[2] != 0.0 for ch in searches[1]["root_children"]),
        "shaping_terms": len(searches[2]["potential_shaping_terms"]) > 0,
    }
    missing = [k for k, v in cover.items() if not v]
    assert not missing, f"coverage missing: {missing} (prob range {min(flat)} .. {max(flat)})"
    for r in recs:
        del r["_legal"], r["_current"]
    doc = {"columns": list(COLUMNS), "max_turns": MAX_TURNS, "training": train,
           "model": WinProbModel.from_pipeline(pipe_full, COLUMNS).to_dict(),
           "model_subset": WinProbModel.from_pipeline(pipe_subset, subset).to_dict(),
           "positions": recs, "search": search_doc, "coverage": cover}
    text = json.dumps(doc, separators=(",", ":"))
    limit = os.path.getsize(os.path.join(GOLDEN, "winprob_features.json"))
    assert len(text) < limit, (len(text), limit)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(f"wrote {OUT}: {len(text)} bytes, {len(recs)} positions, search at position {at} "
          f"(player {player_value}, {searches[0]['n_legal']} legal moves), reference seconds "
          f"{[s['reference_seconds'] for s in searches]}")


if __name__ == "__main__":
    main()
