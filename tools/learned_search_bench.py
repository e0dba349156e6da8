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


def single(fix, model_path, iterations, warmup, repeats, bias):
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
    times = {"exact": [], "leaf": []}
    moves = {}
    for rep in range(warmup + repeats):
        for backend in ("exact", "leaf"):  # alternating
            agent = MCTSAgent(iterations=iterations, rollout_agent=RandomAgent(seed=9001), seed=9002,
                              learned_model_path=model_path, leaf_evaluation_enabled=True,
                              progressive_bias_enabled=bias, rollout_backend=backend)
            t0 = time.perf_counter()
            moves[backend] = agent.select_action(board, player, legal)
            dt = time.perf_counter() - t0
            if rep >= warmup:
                times[backend].append(dt)
    ex, lf = spread(times["exact"]), spread(times["leaf"])
    return {"tool": "learned_search_bench", "what": "one search, wall time of select_action", "iterations": iterations,
            "progressive_bias": bias, "n_legal": len(legal), "warmup": warmup, "exact": ex, "leaf": lf,
            "exact_over_leaf": ex["median_s"] / lf["median_s"], "same_move": move_to_int(moves["exact"]) == move_to_int(moves["leaf"])}


def batch(fix, searches, iterations, warmup, repeats, bias_w):
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
    ms = []
    for rep in range(warmup + repeats):
        d["ttv"].fill_(float("nan"))  # an empty TT per launch
        d["ttc"].zero_()
        gpu.mcts_learned_device(d["roots"], d["sets"], d["pl"], None, d["zob"], d["zidx"], d["log"], d["nodes"], d["out"],
                                model, d["bias"], iterations=iterations, max_turns=int(fix["max_turns"]),
                                bias_weight=bias_w, prior_bias=d["prior"], tt_keys=d["ttk"], tt_vals=d["ttv"],
                                tt_count=d["ttc"])
        if rep >= warmup:
            ms.append(gpu.last_kernel_ms())
    out = d["out"].cpu().numpy().view(N.MCTS_OUT_DTYPE).reshape(n)
    med = statistics.median(ms) / 1e3
    evals = int(out["rollouts"].astype(np.int64).sum()) + int(d["bias"].sum().item())
    return {"tool": "learned_search_bench", "what": "leaf searches in one launch (HIP events)", "kernel": gpu.last_kernel(),
            "searches": n, "iterations": iterations, "bias_weight": bias_w, "distinct_roots": k, "warmup": warmup,
            "launch": spread([m / 1e3 for m in ms]), "searches_per_s": n / med,
            "simulations_per_s": int(out["iterations_run"].astype(np.int64).sum()) / med,
            "leaf_evaluations": evals, "leaf_evaluations_per_s": evals / med,
            "tt_hits": int(out["tt_hits"].astype(np.int64).sum()), "k_winprob_boards_per_s": 75e6}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iterations", type=int, nargs="*", default=[24, 256])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--searches", type=int, default=1024)
    ap.add_argument("--batch-iterations", type=int, default=256)
    ap.add_argument("--bias", action="store_true", help="progressive bias on (weight 0.25)")
    ap.add_argument("--skip-single", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    fix = fixture()
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
