#!/usr/bin/env python3
"""Kernel time of the heuristic playout kernels alone (diagnostic A/B, GPU box): `--games`
(4,096) all-heuristic arena games from the empty board, per-seat numpy streams, `--reps`
launches of each kernel after one warm-up each, the two kernels alternating in one process,
timed with HIP events (bk_last_kernel_ms):

* k_rollout_fr_h  -- bk_rollout_frontier, the default weights compiled in;
* k_rollout_fr_hw -- bk_rollout_frontier_w with four sets that are all the default
  weights and a different seat-to-set byte per game, so the games are the same games
  (the results are compared byte for byte).

`--only h` times the first kernel alone: a library built from a commit without
bk_rollout_frontier_w (BK_LIB_PATH) is measured that way.  One JSON line per kernel, then
one with the ratio of the medians.

`--arena N [--host-games K]`: games/s of run_experiment on the fixtures' arena_pure run
config instead (see arena())."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def arena(games, host_games, reps):
    """games/s of run_experiment on the fixtures' arena_pure config (heuristic A, heuristic
    B, default heuristic, random; round robin): `games` games batched (median of `reps`
    runs after a warm-up) against `host_games` games through the host loop (one launch
    per ply, what such a config got before the weight sets were batched)."""
    import tempfile
    import time

    from reinforcementlearning_blokus_amd.arena import RunConfig, run_experiment
    with open(os.path.join(ROOT, "tests", "golden", "heuristic_weights.json")) as f:
        conf = json.load(f)["arena_pure_config"]
    with tempfile.TemporaryDirectory() as tmp:
        def run(n, batched):
            cfg = RunConfig.from_dict(dict(conf, num_games=n, output_root=tmp))
            t0 = time.perf_counter()
            run_experiment(cfg, batched=batched)
            return time.perf_counter() - t0
        run(64, True)
        secs = [run(games, True) for _ in range(reps)]
        host = run(host_games, False)
    b, h = games / statistics.median(secs), host_games / host
    print(json.dumps({"config": "arena_pure", "batched_games": games, "batched_s": [round(x, 4) for x in secs],
                      "batched_games_per_s": b, "host_loop_games": host_games, "host_loop_s": host,
                      "host_loop_games_per_s": h, "host_loop_s_scaled_to_batched_games": host * games / host_games,
                      "speedup": b / h}), flush=True)


def main():
    if "--arena" in sys.argv:
        return arena(_arg("--arena", 1024), _arg("--host-games", 8), _arg("--reps", 3))
    games, reps, only = _arg("--games", 4096), _arg("--reps", 10), _arg("--only", "")
    from reinforcementlearning_blokus_amd import _native as N
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU, empty_state
    gpu = BlokusGPU(0)
    seeds = (np.arange(games * 4, dtype=np.uint32).reshape(games, 4) * 2654435761 + 20260311).astype(np.uint32)
    kw = dict(semantics=N.SEM_ARENA, rng=N.RNG_NUMPY_MT, compat_seeds=seeds, root_index=np.zeros(games, np.int32),
              heuristic_seats=0xF)
    plans = {"h": {}}
    if only != "h":
        plans["hw"] = {"heur_sets": [N.HEUR_DEFAULT_WEIGHTS] * 4,
                       "seat_sets": ((np.arange(games) * 37 + 11) & 0xFF).astype(np.uint8)}
    med, res, times, names = {}, {}, {tag: [] for tag in plans}, {}
    for _ in range(reps + 1):  # (the first round is the warm-up)
        for tag, plan in plans.items():
            res[tag] = gpu.rollout_frontier(empty_state(), N.fset_new(1), games, **kw, **plan)
            times[tag].append(gpu.last_kernel_ms())
            names[tag] = gpu.last_kernel()
    for tag in plans:
        ms = times[tag][1:]
        med[tag] = statistics.median(ms)
        print(json.dumps({"kernel": names[tag], "games": games, "plies": int(res[tag]["plies"].sum()),
                          "uncertified": int(np.count_nonzero(res[tag]["status"] & N.STATUS_UNCERT)),
                          "ms": [round(x, 4) for x in ms], "ms_min": min(ms), "ms_median": med[tag]}), flush=True)
    if len(med) == 2:
        print(json.dumps({"ratio_hw_over_h": med["hw"] / med["h"],
                          "same_results": res["h"].tobytes() == res["hw"].tobytes()}), flush=True)


if __name__ == "__main__":
    main()
