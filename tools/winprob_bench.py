#!/usr/bin/env python3
"""bk_snapshot_features throughput: the win-probability snapshot rows (four players, 34
columns) of a batch of mid-game boards in one launch.

Positions: --boards (default 4,096) boards spread evenly over plies --min-ply..--max-ply
(default 8..40), played from the empty board on the GPU (bk_rollout_frontier,
BK_SEM_ADVANCE) so each comes with its frontier tables -- the batch tools/telemetry_bench.py
times.  After --warmup launches the same batch is launched --launches times (>= 10) from
device tensors, records and feature matrix both written; each launch is timed by the
library's HIP events around k_snapshot (bk_last_kernel_ms).  One JSON line: boards/s from
the median launch, and the spread (min / max / relative half-range).  --with-telemetry
also times bk_telemetry (stability on, k = 3) on the same tensors in the same process,
the launches of the two kernels alternating.  --eval times bk_winprob_eval instead (the
learned evaluator, k_winprob: device pointers, no pair logits; the model from --model),
alternating with bk_snapshot_features writing the rows only, and reports both medians and
their ratio.  --gbt times bk_winprob_eval_gbt (k_winprob_gbt, a pairwise_gbt_phase model)
alternating with bk_winprob_eval on the same tensors, once per entry of --gbt-stages: the
model of --gbt-model as it is (40 stages per phase in the fixture), or with every ensemble's
trees repeated up to that many stages, so the cost per stage shows.  One JSON line per entry,
appended to --out when given.

The comparison point is the reference's build_snapshot_runtime_context +
extract_player_snapshot_features for the four players on one CPU core over the same ply
range (profiles/winprob/README.md has the measured pair); this tool never compares
against the code under test.  --cpu-reference PATH times the reference checkout at PATH
on this machine's CPU instead (no GPU call; positions from generate_random_valid_state
over the same plies).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_reference(path: str, calls: int, lo: int, hi: int) -> dict:
    sys.path.insert(0, path)
    from analytics.winprob.features import build_snapshot_runtime_context, extract_player_snapshot_features
    from engine.board import Player
    from engine.move_generator import LegalMoveGenerator
    from tests.utils_game_states import generate_random_valid_state
    mg = LegalMoveGenerator()
    times = []
    for i in range(calls):
        ply = lo + (i * (hi - lo)) // max(1, calls - 1)
        board, _ = generate_random_valid_state(ply, 1000 + i)
        t0 = time.perf_counter()
        ctx = build_snapshot_runtime_context(board, turn_index=ply, max_turns=2500)
        for p in Player:
            extract_player_snapshot_features(board, player=p, context=ctx, move_generator=mg)
        times.append(time.perf_counter() - t0)
    return {"tool": "winprob_bench", "what": "reference snapshot rows of one board (context + 4 players), one CPU core",
            "calls": calls, "min_ply": lo, "max_ply": hi, "boards_per_s": calls / sum(times),
            "median_s": statistics.median(times), "min_s": min(times), "max_s": max(times)}


def eval_bench(gpu, args, d_st, d_fs, d_ti, n) -> dict:
    """bk_winprob_eval (device pointers, no pair logits) and bk_snapshot_features writing the
    rows only, alternating in this process on the same tensors; each launch timed by the
    library's HIP events around it."""
    import torch

    from reinforcementlearning_blokus_amd.mcts.learned_evaluator import WinProbModel
    with open(args.model) as fh:
        doc = json.load(fh)
    model = WinProbModel.from_dict(doc.get("model", doc))
    ev_ms, sn_ms = [], []
    for i in range(args.warmup + args.launches):
        prob, _, status = gpu.winprob_eval(d_st, d_fs, d_ti, 2500, model)
        gpu.synchronize()
        assert gpu.last_kernel() == "k_winprob"
        if i >= args.warmup:
            ev_ms.append(gpu.last_kernel_ms())
        _, feat = gpu.snapshot_features(d_st, d_fs, d_ti, 2500, records=False)
        gpu.synchronize()
        assert gpu.last_kernel() == "k_snapshot"
        if i >= args.warmup:
            sn_ms.append(gpu.last_kernel_ms())
    torch.cuda.synchronize()
    prob = prob.cpu().numpy()
    emed, smed = statistics.median(ev_ms), statistics.median(sn_ms)
    return {"tool": "winprob_bench", "mode": "eval", "boards": n, "min_ply": args.min_ply, "max_ply": args.max_ply,
            "warmup": args.warmup, "launches": len(ev_ms),
            "winprob_ms_median": emed, "winprob_ms_min": min(ev_ms), "winprob_ms_max": max(ev_ms),
            "winprob_spread_rel": (max(ev_ms) - min(ev_ms)) / (2 * emed),
            "snapshot_rows_ms_median": smed, "snapshot_rows_ms_min": min(sn_ms), "snapshot_rows_ms_max": max(sn_ms),
            "snapshot_rows_spread_rel": (max(sn_ms) - min(sn_ms)) / (2 * smed),
            "winprob_over_snapshot_rows": emed / smed, "boards_per_s": n / (emed * 1e-3),
            "evaluations_per_s": 4 * n / (emed * 1e-3), "status_nonzero": int(status.cpu().numpy().astype(bool).sum()),
            "prob_finite": bool(np.isfinite(prob).all()), "prob_mean": float(prob.mean())}


def stretched(model, stages):
    """`model` with every ensemble's trees repeated (whole copies of its node array) until it
    has `stages` stages; the learning rate shrinks alike, so the scores stay in range."""
    from reinforcementlearning_blokus_amd.mcts.learned_evaluator import GbtEnsemble, GbtPhaseModel
    out = []
    for e in model.ensembles:
        reps = -(-stages // len(e.roots))
        n = len(e.tv)
        roots = [r + k * n for k in range(reps) for r in e.roots][:stages]
        left = [lf if lf == -1 else lf + k * n for k in range(reps) for lf in e.left]
        out.append(GbtEnsemble(e.init, e.learning_rate * len(e.roots) / stages, roots, left, e.feature * reps, e.tv * reps))
    return GbtPhaseModel(out, model.phase_ensemble, model.mean, model.scale, model.feature_columns)


def gbt_bench(gpu, args, d_st, d_fs, d_ti, n) -> list:
    """bk_winprob_eval_gbt and bk_winprob_eval (device pointers, no pair outputs) alternating in
    this process on the same tensors; each launch timed by the library's HIP events."""
    import torch

    from reinforcementlearning_blokus_amd.mcts.learned_evaluator import GbtPhaseModel, WinProbModel
    with open(args.model) as fh:
        doc = json.load(fh)
    logreg = WinProbModel.from_dict(doc.get("model", doc))
    with open(args.gbt_model) as fh:
        doc = json.load(fh)
    base = GbtPhaseModel.from_dict(doc["models"]["phases"] if "models" in doc else doc)
    lines = []
    for stages in args.gbt_stages:
        model = base if all(len(e.roots) == stages for e in base.ensembles) else stretched(base, stages)
        gbt_ms, lr_ms = [], []
        for i in range(args.warmup + args.launches):
            _, _, _ = gpu.winprob_eval(d_st, d_fs, d_ti, 2500, logreg)
            gpu.synchronize()
            assert gpu.last_kernel() == "k_winprob"
            if i >= args.warmup:
                lr_ms.append(gpu.last_kernel_ms())
            prob, _, status = gpu.winprob_eval_gbt(d_st, d_fs, d_ti, 2500, model)
            gpu.synchronize()
            assert gpu.last_kernel() == "k_winprob_gbt"
            if i >= args.warmup:
                gbt_ms.append(gpu.last_kernel_ms())
        torch.cuda.synchronize()
        prob = prob.cpu().numpy()
        gmed, lmed = statistics.median(gbt_ms), statistics.median(lr_ms)
        lines.append({"tool": "winprob_bench", "mode": "gbt", "boards": n, "min_ply": args.min_ply,
                      "max_ply": args.max_ply, "warmup": args.warmup, "launches": len(gbt_ms), "stages": stages,
                      "nodes": sum(len(e.tv) for e in model.ensembles), "ensembles": len(model.ensembles),
                      "gbt_ms_median": gmed, "gbt_ms_min": min(gbt_ms), "gbt_ms_max": max(gbt_ms),
                      "gbt_spread_rel": (max(gbt_ms) - min(gbt_ms)) / (2 * gmed),
                      "logreg_ms_median": lmed, "logreg_ms_min": min(lr_ms), "logreg_ms_max": max(lr_ms),
                      "logreg_spread_rel": (max(lr_ms) - min(lr_ms)) / (2 * lmed),
                      "gbt_over_logreg": gmed / lmed, "boards_per_s": n / (gmed * 1e-3),
                      "evaluations_per_s": 4 * n / (gmed * 1e-3),
                      "status_nonzero": int(status.cpu().numpy().astype(bool).sum()),
                      "prob_finite": bool(np.isfinite(prob).all()), "prob_mean": float(prob.mean())})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--min-ply", type=int, default=8)
    ap.add_argument("--max-ply", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--with-telemetry", action="store_true", help="also time bk_telemetry on the same boards")
    ap.add_argument("--eval", action="store_true",
                    help="time bk_winprob_eval (no pair logits) alternating with bk_snapshot_features (rows only)")
    ap.add_argument("--model", metavar="JSON", default=os.path.join(ROOT, "tests", "golden", "winprob_eval.json"),
                    help="--eval: a WinProbModel JSON document, or a fixture holding one under \"model\"")
    ap.add_argument("--gbt", action="store_true",
                    help="time bk_winprob_eval_gbt alternating with bk_winprob_eval, once per --gbt-stages entry")
    ap.add_argument("--gbt-model", metavar="JSON", default=os.path.join(ROOT, "tests", "golden", "winprob_gbt.json"),
                    help="--gbt: a GbtPhaseModel JSON document, or a fixture holding one under models.phases")
    ap.add_argument("--gbt-stages", type=int, nargs="+", default=[40, 400])
    ap.add_argument("--out", metavar="JSONL", help="--gbt: also append the lines to this file")
    ap.add_argument("--cpu-reference", metavar="PATH", help="time the reference checkout at PATH on the CPU instead")
    ap.add_argument("--cpu-calls", type=int, default=33)
    args = ap.parse_args()
    if args.cpu_reference:
        print(json.dumps(cpu_reference(args.cpu_reference, args.cpu_calls, args.min_ply, args.max_ply)), flush=True)
        return
    if args.launches < 10:
        ap.error("--launches must be at least 10")
    import torch

    from reinforcementlearning_blokus_amd import _native as N
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU, empty_state
    gpu = BlokusGPU(0)
    plies = list(range(args.min_ply, args.max_ply + 1))
    per = [args.boards // len(plies) + (1 if i < args.boards % len(plies) else 0) for i in range(len(plies))]
    states, sets = [], []
    for ply, cnt in zip(plies, per):
        if cnt == 0:
            continue
        st, fs = gpu.rollout_frontier(empty_state(), N.fset_new(1), cnt, semantics=N.SEM_ADVANCE, rng=N.RNG_PHILOX,
                                      seed=args.seed + ply, max_plies=ply, root_index=np.zeros(cnt, dtype=np.int32))
        states.append(st)
        sets.append(fs)
    states, sets = np.concatenate(states), np.concatenate(sets)
    n = len(states)
    dev = torch.device("cuda", 0)
    d_st = torch.from_numpy(states.view(np.uint8).reshape(n, 256).copy()).to(dev)
    d_fs = torch.from_numpy(sets.view(np.uint8).reshape(n, N.FSET_DTYPE.itemsize).copy()).to(dev)
    d_ti = torch.from_numpy(states["move_count"].astype(np.int32)).to(dev)
    if args.eval:
        print(json.dumps(eval_bench(gpu, args, d_st, d_fs, d_ti, n)), flush=True)
        return
    if args.gbt:
        for line in gbt_bench(gpu, args, d_st, d_fs, d_ti, n):
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")
        return
    ms, tel_ms = [], []
    for i in range(args.warmup + args.launches):
        rec, feat = gpu.snapshot_features(d_st, d_fs, d_ti, 2500)
        gpu.synchronize()
        if i >= args.warmup:
            ms.append(gpu.last_kernel_ms())
        if args.with_telemetry:
            gpu.telemetry(d_st, d_fs, k_samples=3)
            gpu.synchronize()
            if i >= args.warmup:
                tel_ms.append(gpu.last_kernel_ms())
    rec = rec.cpu().numpy().view(N.SNAPSHOT_REC_DTYPE).reshape(n, 4)
    feat = feat.cpu().numpy()
    med = statistics.median(ms)
    out = {
        "tool": "winprob_bench", "kernel": "k_snapshot", "boards": n, "min_ply": args.min_ply,
        "max_ply": args.max_ply, "warmup": args.warmup, "launches": len(ms),
        "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
        "spread_rel": (max(ms) - min(ms)) / (2 * med), "boards_per_s": n / (med * 1e-3),
        "rows_per_s": 4 * n / (med * 1e-3), "move_generations_per_s": 4 * n / (med * 1e-3),
        "status_nonzero": int((rec["status"] != 0).sum()), "mean_mobility": float(rec["mobility"].mean()),
        "mean_deadzone_count": float(rec["deadzone_count"].mean()),
        "features_finite": bool(np.isfinite(feat).all()),
    }
    if tel_ms:
        tmed = statistics.median(tel_ms)
        out.update(telemetry_ms_median=tmed, telemetry_ms_min=min(tel_ms), telemetry_ms_max=max(tel_ms),
                   snapshot_over_telemetry=med / tmed)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
