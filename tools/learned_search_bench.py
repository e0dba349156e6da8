#!/usr/bin/env python3
"""Learned MCTSAgent searches: the ``exact`` backend (host tree, one bk_winprob_eval launch
per evaluation) against the ``leaf`` backend (the whole search in one bk_mcts_learned launch,
k_mcts_coop_l), and the leaf backend's batch throughput.

Positions and model come from tests/golden/winprob_eval.json (data; nothing is compared
against the code under test here -- tests/test_gpu_mcts_leaf.py does that).

* single: the fixture's search position, leaf evaluation with the TT on, a fresh agent per
  search; after --warmup searches of each backend, --repeats (>= 10) searches of each,
  alternating in this one process.  Wall time of select_action per search: median, min, max.
  One JSON line per iteration count (--iterations, default 24 and 256).
* batch: --searches (default 1,024) leaf searches of --batch-iterations (256) iterations in
  one launch from device tensors, the roots the fixture positions where some player has >= 2
  legal moves, cycled; timed by the library's HIP events around the kernel
  (bk_last_kernel_ms), median of --repeats launches after --warmup.  Reports searches/s and
  leaf evaluations/s; k_winprob alone evaluates about 75 M boards/s, the
  ceiling for the evaluations.
* --gbt: the tree-model mode, same protocol.  The ``leaf_gbt`` backend (bk_mcts_learned_gbt,
  k_mcts_coop_g) with the ``phases`` model of tests/golden/winprob_gbt.json is measured against
  the ``exact`` backend with that model and against the logistic ``leaf`` launch, all three
  alternating in this one process: one line per iteration count and bias setting for the single
  search, one line per bias setting for the batch (the tree and the logistic launch alternate).
  Bias off and weight 0.25 both run.
"""
from __future__ import annotations

import argparse
import base64
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "winprob_eval.json")) as fh:
        return json.load(fh)


def spread(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "n": len(xs)}


def single(fix, model_path, iterations, warmup, repeats, bias, contenders=None):
    """contenders: (label, rollout_backend, model path) of the searches that alternate; the
    default is the logistic model's exact and leaf backends."""
    from reinforcementlearning_blokus_amd.agents.random_agent import RandomAgent
    from reinforcementlearning_blokus_amd.engine.board import Board, Player, Position
    from reinforcementlearning_blokus_amd.engine.move_generator import get_shared_generator, move_to_int
    from reinforcementlearning_blokus_amd.mcts.mcts_agent import MCTSAgent
    s = fix["search"]
    board = Board()
    for player_value, piece_id, cells in s["log"]:
        board.current_player = Player(player_value)
        board.place_piece([Position(r, c) for r, c in cells], Player(player_value), piece_id, validate=False)
    board.current_player = Player(s["current_player"])
    player = Player(s["player"])
    legal = get_shared_generator().get_legal_moves(board, player)
    contenders = contenders or [("exact", "exact", model_path), ("leaf", "leaf", model_path)]
    times = {label: [] for label, _, _ in contenders}
    moves = {}
    for rep in range(warmup + repeats):
        for label, backend, path in contenders:  # alternating
            agent = MCTSAgent(iterations=iterations, rollout_agent=RandomAgent(seed=9001), seed=9002,
                              learned_model_path=path, leaf_evaluation_enabled=True,
                              progressive_bias_enabled=bias, rollout_backend=backend)
            t0 = time.perf_counter()
            moves[label] = agent.select_action(board, player, legal)
            dt = time.perf_counter() - t0
            if rep >= warmup:
                times[label].append(dt)
    doc = {"tool": "learned_search_bench", "what": "one search, wall time of select_action", "iterations": iterations,
           "progressive_bias": bias, "n_legal": len(legal), "warmup": warmup}
    doc.update({label: spread(times[label]) for label in times})
    if "leaf_gbt" in times:  # the tree model: its two backends must agree, the logistic launch is the yardstick
        doc.update(model="pairwise_gbt_phase (phases)",
                   exact_over_leaf_gbt=doc["exact"]["median_s"] / doc["leaf_gbt"]["median_s"],
                   leaf_gbt_over_leaf=doc["leaf_gbt"]["median_s"] / doc["leaf"]["median_s"],
                   same_move=move_to_int(moves["exact"]) == move_to_int(moves["leaf_gbt"]))
    else:
        doc.update(exact_over_leaf=doc["exact"]["median_s"] / doc["leaf"]["median_s"],
                   same_move=move_to_int(moves["exact"]) == move_to_int(moves["leaf"]))
    return doc


def batch(fix, searches, iterations, warmup, repeats, bias_w, gbt_model=None):
    """gbt_model: also launch the searches with this tree model, alternating with the logistic
    launch; the result then describes the tree launch and carries the logistic one beside it."""
    import torch

    from reinforcementlearning_blokus_amd import _native as N
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU, mcts_log_table, mcts_node_cap
    from reinforcementlearning_blokus_amd.mcts.learned_evaluator import WinProbModel
    from reinforcementlearning_blokus_amd.mcts.zobrist import ZobristHash, flat_keys
    dec = lambda text, dt: np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype=dt).copy()  # noqa: E731
    roots, sets, players = [], [], []
    for r in fix["positions"]:
        mob = [int(r["rows"][p][6]) for p in range(4)]  # mobility_total_placements: legal moves
        movers = [p for p in range(4) if mob[p] >= 2]
        if movers:
            roots.append(dec(r["state"], N.STATE_DTYPE))
            sets.append(dec(r["sets"], N.FSET_DTYPE))
            players.append(movers[0])
    k = len(roots)
    pick = [i % k for i in range(searches)]
    rts = np.concatenate([roots[i] for i in pick])
    sts = np.concatenate([sets[i] for i in pick])
    pl = np.array([players[i] for i in pick], np.uint8)
    rts["current_player"] = pl
    gpu = BlokusGPU.shared(0)
    dev = "cuda:0"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    n, cap, tt_cap = searches, mcts_node_cap(iterations), 1 << max(4, (2 * (iterations + 2) - 1).bit_length())
    d = dict(roots=up(rts.view(np.uint8).reshape(n, 256)), sets=up(sts.view(np.uint8).reshape(n, -1)), pl=up(pl),
             zob=up(flat_keys(ZobristHash(seed=9002)).view(np.int64).reshape(1, -1)),
             zidx=torch.zeros(n, dtype=torch.int32, device=dev), log=up(mcts_log_table(iterations)),
             nodes=torch.empty((n, cap * N.MCTS_NODE_DTYPE.itemsize), dtype=torch.uint8, device=dev),
             out=torch.zeros((n, N.MCTS_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev),
             prior=torch.zeros((n, cap), dtype=torch.float64, device=dev),
             bias=torch.zeros(n, dtype=torch.int32, device=dev),
             ttk=torch.zeros((n, tt_cap), dtype=torch.int64, device=dev),
             ttv=torch.empty((n, tt_cap), dtype=torch.float64, device=dev),
             ttc=torch.zeros(n, dtype=torch.int32, device=dev))
    model = WinProbModel.from_dict(fix["model"])
    ms, ms_logreg, kernel = [], [], ""
    for rep in range(warmup + repeats):
        for m in ([model, gbt_model] if gbt_model is not None else [model]):  # the measured launch last: `out` is its
            d["ttv"].fill_(float("nan"))  # an empty TT per launch
            d["ttc"].zero_()
            gpu.mcts_learned_device(d["roots"], d["sets"], d["pl"], None, d["zob"], d["zidx"], d["log"], d["nodes"],
                                    d["out"], m, d["bias"], iterations=iterations, max_turns=int(fix["max_turns"]),
                                    bias_weight=bias_w, prior_bias=d["prior"], tt_keys=d["ttk"], tt_vals=d["ttv"],
                                    tt_count=d["ttc"])
            if rep >= warmup:
                (ms if m is not model or gbt_model is None else ms_logreg).append(gpu.last_kernel_ms())
            kernel = gpu.last_kernel()
    out = d["out"].cpu().numpy().view(N.MCTS_OUT_DTYPE).reshape(n)
    med = statistics.median(ms) / 1e3
    evals = int(out["rollouts"].astype(np.int64).sum()) + int(d["bias"].sum().item())
    doc = {"tool": "learned_search_bench", "what": "leaf searches in one launch (HIP events)", "kernel": kernel,
           "searches": n, "iterations": iterations, "bias_weight": bias_w, "distinct_roots": k, "warmup": warmup,
           "launch": spread([m / 1e3 for m in ms]), "searches_per_s": n / med,
           "simulations_per_s": int(out["iterations_run"].astype(np.int64).sum()) / med,
           "leaf_evaluations": evals, "leaf_evaluations_per_s": evals / med,
           "tt_hits": int(out["tt_hits"].astype(np.int64).sum()), "k_winprob_boards_per_s": 75e6}
    if gbt_model is not None:
        del doc["k_winprob_boards_per_s"]  # (the logistic evaluator's ceiling)
        lg = statistics.median(ms_logreg) / 1e3
        doc.update(model="pairwise_gbt_phase (phases)", logreg_launch=spread([m / 1e3 for m in ms_logreg]),
                   logreg_searches_per_s=n / lg, gbt_over_logreg_launch=med / lg)
    return doc


def main_gbt(a, fix):
    from reinforcementlearning_blokus_amd.mcts.learned_evaluator import GbtPhaseModel
    with open(os.path.join(ROOT, "tests", "golden", "winprob_gbt.json")) as fh:
        phases = json.load(fh)["models"]["phases"]
    with tempfile.TemporaryDirectory() as tmp:
        logreg_path, gbt_path = os.path.join(tmp, "model.json"), os.path.join(tmp, "gbt.json")
        for path, doc in ((logreg_path, fix["model"]), (gbt_path, phases)):
            with open(path, "w") as fh:
                json.dump(doc, fh)
        contenders = [("exact", "exact", gbt_path), ("leaf_gbt", "leaf_gbt", gbt_path), ("leaf", "leaf", logreg_path)]
        single_lines = []
        if not a.skip_single:
            for bias in (False, True):
                for it in a.iterations:
                    single_lines.append(single(fix, gbt_path, it, a.warmup, a.repeats, bias, contenders))
                    print(json.dumps(single_lines[-1]), flush=True)
    if not a.skip_batch:
        model = GbtPhaseModel.from_dict(phases)
        for bias_w in (0.0, 0.25):
            doc = batch(fix, a.searches, a.batch_iterations, a.warmup, a.repeats, bias_w, model)
            for s in single_lines:  # what one exact search costs in batched leaf_gbt searches
                if s["iterations"] == a.batch_iterations and s["progressive_bias"] == (bias_w != 0.0):
                    doc["exact_search_in_batched_searches"] = s["exact"]["median_s"] * doc["searches_per_s"]
            print(json.dumps(doc), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iterations", type=int, nargs="*", default=[24, 256])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--searches", type=int, default=1024)
    ap.add_argument("--batch-iterations", type=int, default=256)
    ap.add_argument("--bias", action="store_true", help="progressive bias on (weight 0.25)")
    ap.add_argument("--gbt", action="store_true", help="the tree-model mode: leaf_gbt against exact and the logistic leaf")
    ap.add_argument("--skip-single", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    fix = fixture()
    if a.gbt:
        return main_gbt(a, fix)
    with tempfile.TemporaryDirectory() as tmp:
        model_path = os.path.join(tmp, "model.json")
        with open(model_path, "w") as fh:
            json.dump(fix["model"], fh)
        if not a.skip_single:
            for it in a.iterations:
                print(json.dumps(single(fix, model_path, it, a.warmup, a.repeats, a.bias)), flush=True)
    if not a.skip_batch:
        print(json.dumps(batch(fix, a.searches, a.batch_iterations, a.warmup, a.repeats, 0.25 if a.bias else 0.0)),
              flush=True)


if __name__ == "__main__":
    main()
