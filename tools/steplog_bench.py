#!/usr/bin/env python3
"""bk_step_metrics throughput: the integers behind the strategy step log for a batch of
(before, move, after) steps in one launch.

Steps: --steps (default 4,096) pairs of boards spread evenly over plies --min-ply..--max-ply
(default 8..40), built on the GPU: the before board is played from the empty board to its
ply (bk_rollout_frontier, BK_SEM_ADVANCE), the after board is the before board advanced by
one more placement, each with its frontier tables; the step (mover, piece, orientation,
anchor) is read off the pair on the host, and a pair without a placement (a finished game)
is dropped.  After --warmup launches the batch is launched --launches times (>= 20) from
device tensors; each launch is timed by the library's HIP events around k_steplog
(bk_last_kernel_ms).  In the same process, the launches alternating, two record-only
bk_snapshot_features launches over the same before and after boards are timed: without
bk_step_metrics that is the cheapest way to the same eight move counts, so it is the
comparison point.  One JSON line: the medians, minima, maxima and relative half-ranges of
both, their ratio, and steps/s from the median launch.

--cpu-reference PATH times the reference checkout's seven metric functions per step (as
its StrategyLogger.on_step calls them) on one CPU core of this machine instead: no GPU
call; positions from generate_random_valid_state over the same plies.  A run that finds no
GPU fails; nothing falls back.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_reference(path: str, calls: int, lo: int, hi: int) -> dict:
    sys.path.insert(0, path)
    from analytics.metrics import (MetricInput, compute_blocking_metrics, compute_center_metrics,
                                   compute_corner_metrics, compute_mobility_metrics, compute_piece_metrics,
                                   compute_proximity_metrics, compute_territory_metrics)
    from analytics.metrics.mobility import get_mobility_counts
    from engine.board import Player
    from engine.move_generator import LegalMoveGenerator
    from tests.utils_game_states import generate_random_valid_state
    mg = LegalMoveGenerator()
    times = []
    for i in range(calls):
        ply = lo + (i * (hi - lo)) // max(1, calls - 1)
        board, _ = generate_random_valid_state(ply, 1000 + i)
        legal = []
        for _ in range(4):
            legal = mg.get_legal_moves(board, board.current_player)
            if legal:
                break
            board._update_current_player()
        if not legal:
            continue
        player, move = board.current_player, random.Random(i).choice(legal)
        state = board.copy()
        positions = move.get_positions(mg.piece_orientations_cache[move.piece_id])
        assert board.place_piece(positions, player, move.piece_id)
        t0 = time.perf_counter()
        inp = MetricInput(state=state, move=move, next_state=board, player_id=player.value,
                          opponents=[p.value for p in Player if p != player],
                          placed_squares=[(p.row, p.col) for p in positions], precomputed_values={})
        before, after = get_mobility_counts(inp)
        inp.precomputed_values["mobility_counts_before"] = before
        inp.precomputed_values["mobility_counts_after"] = after
        for fn in (compute_center_metrics, compute_territory_metrics, compute_mobility_metrics,
                   compute_blocking_metrics, compute_corner_metrics, compute_proximity_metrics, compute_piece_metrics):
            fn(inp)
        times.append(time.perf_counter() - t0)
    return {"tool": "steplog_bench", "what": "reference step metrics of one step (7 functions, 8 generations), one CPU core",
            "calls": len(times), "min_ply": lo, "max_ply": hi, "steps_per_s": len(times) / sum(times),
            "median_s": statistics.median(times), "min_s": min(times), "max_s": max(times)}


def steps_of(before, after, orient_table) -> tuple:
    """The step of each (before, after) pair, read off the boards: STEP_DTYPE[n] and the mask of
    pairs that hold exactly one placement."""
    from reinforcementlearning_blokus_amd import _native as N
    by_cells = {}
    for pid, o, offs in orient_table:
        by_cells[(pid, tuple(sorted((int(r), int(c)) for r, c in offs)))] = o
    steps = np.zeros(len(before), dtype=N.STEP_DTYPE)
    keep = np.zeros(len(before), dtype=bool)
    for i in range(len(before)):
        new_used = after["used"][i] & ~before["used"][i]
        movers = np.nonzero(new_used)[0]
        if len(movers) != 1 or int(after["move_count"][i]) != int(before["move_count"][i]) + 1:
            continue
        m = int(movers[0])
        piece = int(new_used[m]).bit_length()
        plane = lambda s: int.from_bytes(s["planes"][i, m].tobytes(), "little")  # noqa: E731
        diff = plane(after) & ~plane(before)
        cells = [(k // 20, k % 20) for k in range(400) if (diff >> k) & 1]
        ar, ac = min(r for r, _ in cells), min(c for _, c in cells)
        o = by_cells[(piece, tuple(sorted((r - ar, c - ac) for r, c in cells)))]
        steps[i] = (m, piece, o, ar, ac, [0, 0, 0])
        keep[i] = True
    return steps, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--min-ply", type=int, default=8)
    ap.add_argument("--max-ply", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--cpu-reference", metavar="PATH", help="time the reference checkout at PATH on the CPU instead")
    ap.add_argument("--cpu-calls", type=int, default=33)
    args = ap.parse_args()
    if args.cpu_reference:
        print(json.dumps(cpu_reference(args.cpu_reference, args.cpu_calls, args.min_ply, args.max_ply)), flush=True)
        return
    if args.launches < 20:
        ap.error("--launches must be at least 20")
    import torch

    from reinforcementlearning_blokus_amd import _native as N
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU, empty_state
    gpu = BlokusGPU(0)  # raises without a GPU
    plies = list(range(args.min_ply, args.max_ply + 1))
    per = [args.steps // len(plies) + (1 if i < args.steps % len(plies) else 0) for i in range(len(plies))]
    states, sets = [], []
    for ply, cnt in zip(plies, per):
        if cnt == 0:
            continue
        st, fs = gpu.rollout_frontier(empty_state(), N.fset_new(1), cnt, semantics=N.SEM_ADVANCE, rng=N.RNG_PHILOX,
                                      seed=args.seed + ply, max_plies=ply, root_index=np.zeros(cnt, dtype=np.int32))
        states.append(st)
        sets.append(fs)
    before, sets_before = np.concatenate(states), np.concatenate(sets)
    after, sets_after = gpu.rollout_frontier(before, sets_before, len(before), semantics=N.SEM_ADVANCE,
                                             rng=N.RNG_PHILOX, seed=args.seed + 1000, max_plies=1,
                                             root_index=np.arange(len(before), dtype=np.int32))
    steps, keep = steps_of(before, after, N.orient_table())
    before, sets_before, after, sets_after, steps = (a[keep] for a in (before, sets_before, after, sets_after, steps))
    n = len(steps)
    dev = torch.device("cuda", 0)
    d_b, d_sb, d_a, d_sa, d_st = (torch.from_numpy(a.view(np.uint8).reshape(n, -1).copy()).to(dev)
                                  for a in (before, sets_before, after, sets_after, steps))
    d_ti = torch.zeros(n, dtype=torch.int32, device=dev)
    ms, snap_ms = [], []
    for i in range(args.warmup + args.launches):
        rec = gpu.step_metrics(d_b, d_sb, d_a, d_sa, d_st)
        gpu.synchronize()
        assert gpu.last_kernel() == "k_steplog"
        if i >= args.warmup:
            ms.append(gpu.last_kernel_ms())
        pair = 0.0
        for st, fs in ((d_b, d_sb), (d_a, d_sa)):
            snap, _ = gpu.snapshot_features(st, fs, d_ti, 2500, features=False)
            gpu.synchronize()
            assert gpu.last_kernel() == "k_snapshot"
            pair += gpu.last_kernel_ms()
        if i >= args.warmup:
            snap_ms.append(pair)
    torch.cuda.synchronize()
    rec = rec.cpu().numpy().view(N.STEP_REC_DTYPE).reshape(n)
    snap = snap.cpu().numpy().view(N.SNAPSHOT_REC_DTYPE).reshape(n, 4)
    med, smed = statistics.median(ms), statistics.median(snap_ms)
    print(json.dumps({
        "tool": "steplog_bench", "kernel": "k_steplog", "steps": n, "dropped": int((~keep).sum()),
        "min_ply": args.min_ply, "max_ply": args.max_ply, "warmup": args.warmup, "launches": len(ms),
        "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
        "spread_rel": (max(ms) - min(ms)) / (2 * med),
        "two_snapshot_ms_median": smed, "two_snapshot_ms_min": min(snap_ms), "two_snapshot_ms_max": max(snap_ms),
        "two_snapshot_spread_rel": (max(snap_ms) - min(snap_ms)) / (2 * smed),
        "steplog_over_two_snapshot": med / smed, "steps_per_s": n / (med * 1e-3),
        "move_generations_per_s": 8 * n / (med * 1e-3), "status_nonzero": int((rec["status"] != 0).sum()),
        "counts_equal_snapshot": bool(np.array_equal(rec["moves_after"], snap["mobility"])),
        "mean_moves_before": float(rec["moves_before"].mean()),
    }), flush=True)


if __name__ == "__main__":
    main()
