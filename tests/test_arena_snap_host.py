"""bk_arena_step_snap's host side, without a GPU: the two symbols and the plan's layout,
the argument checks that return before any device is touched, the checkpoint-to-mask and
slot helpers, and run_experiment's routing of snapshot runs to the batched driver."""
import ctypes as C
import os
import re

import pytest

from reinforcementlearning_blokus_amd import _native as N
from reinforcementlearning_blokus_amd.arena import RunConfig, game_seed_from_run_seed
from reinforcementlearning_blokus_amd.arena.config import seat_assignment_for_game
from tests.conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "blokus_hip.h")).read()


def test_symbols_and_plan_layout():
    assert "bk_arena_step_snap" in N.EXPORTS and "bk_snap_plan_size" in N.EXPORTS
    lib = N.load()
    assert hasattr(lib, "bk_arena_step_snap") and hasattr(lib, "bk_snap_plan_size")
    assert lib.bk_snap_plan_size() == C.sizeof(N.BkSnapPlan) == 40
    # the header's fields, in order: a 128-bit mask, then three pointers
    body = re.search(r"typedef struct bk_snap_plan \{(.*?)\} bk_snap_plan;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == [f for f, _ in N.BkSnapPlan._fields_]
    assert N.BkSnapPlan.ply_mask.offset == 0 and N.BkSnapPlan.ply_mask.size == 16
    assert [getattr(N.BkSnapPlan, f).offset for f in ("states", "sets", "turn")] == [16, 24, 32]


def test_abi_version_is_unchanged():
    assert N.load().bk_abi_version() == 7 == N.ABI_VERSION
    assert re.search(r"#define BK_ABI_VERSION (\d+)", HEADER).group(1) == "7"


def _call(plan, mem=N.MEM_DEVICE, states=0x1000, h=None):
    """bk_arena_step_snap with made-up, never dereferenced pointers; h None: no handle, no device."""
    cfg = N.BkRolloutCfg(N.SEM_ARENA, N.ORDER_FRONTIER, N.RNG_NUMPY_MT, 2500, 0, 0, 0)
    vp = C.c_void_p
    return N.load().bk_arena_step_snap(h, vp(states), vp(0x2000), 4, C.byref(cfg), vp(0x3000), vp(0), vp(0), vp(0x4000),
                                       vp(0x5000), vp(0), C.byref(plan) if plan is not None else None, mem)


def _plan(mask=(1 << 8, 0, 0, 0), states=0x10000, sets=0x20000, turn=0x30000):
    return N.BkSnapPlan((C.c_uint32 * 4)(*mask), states, sets, turn)


def test_argument_checks_touch_no_device():
    """Every rejected call returns BK_EINVAL before the handle is used: with no handle at
    all (this machine has no GPU) nothing is dereferenced and nothing is launched."""
    assert _call(None) == N.EINVAL                                  # a null plan
    assert _call(_plan(), mem=N.MEM_HOST) == N.EINVAL               # the slots live on the device
    assert _call(_plan(mask=(0, 0, 0, 0))) == N.EINVAL              # an empty mask
    assert _call(_plan(mask=(1 | 1 << 8, 0, 0, 0))) == N.EINVAL     # ply 0 is the caller's
    assert _call(_plan(states=0)) == N.EINVAL and _call(_plan(sets=0)) == N.EINVAL
    assert _call(_plan(turn=0)) == N.EINVAL
    assert _call(_plan(sets=0x20008)) == N.EINVAL                   # sets not 16-byte aligned
    assert _call(_plan(), states=0) == N.EINVAL


def test_checkpoints_to_mask_and_slots():
    assert N.snap_plan_plies([0, 8, 40, 64]) == [8, 40, 64]  # ply 0 is the driver's
    assert N.snap_plan_mask([0, 8, 40, 64]) == [1 << 8, 1 << 8, 1 << 0, 0]
    assert [N.snap_plan_slot([0, 8, 40, 64], c) for c in (8, 40, 64)] == [0, 1, 2]
    assert N.snap_plan_slot([0, 8, 40, 64], 0) == -1 and N.snap_plan_slot([0, 8, 40, 64], 9) == -1
    # duplicates count once, plies a game cannot reach are dropped, slots ascend with the ply
    cps = [64, 8, 8, 127, 128, 500, 2, 64, 0, 31, 32, 96]
    assert N.snap_plan_plies(cps) == [2, 8, 31, 32, 64, 96, 127]
    assert [N.snap_plan_slot(cps, c) for c in N.snap_plan_plies(cps)] == list(range(7))
    mask = N.snap_plan_mask(cps)
    assert mask == [1 << 2 | 1 << 8 | 1 << 31, 1 << 0, 1 << 0, 1 << 0 | 1 << 31]
    # the kernel's rule: the slot of ply c is the number of mask bits below c
    wide = sum(m << (32 * i) for i, m in enumerate(mask))
    for c in N.snap_plan_plies(cps):
        assert bin(wide & ((1 << c) - 1)).count("1") == N.snap_plan_slot(cps, c)
    assert N.snap_plan_plies([]) == [] and N.snap_plan_mask([0, 128]) == [0, 0, 0, 0]
    assert N.snap_plan_mask(range(1, 85)) == [0xFFFFFFFE, 0xFFFFFFFF, 0x1FFFFF, 0]


def _config(tmp_path, fast_params=None, snapshots=True):
    return RunConfig.from_dict({"agents": [
        {"name": "r", "type": "random"}, {"name": "h", "type": "heuristic"},
        {"name": "m", "type": "mcts", "params": {"iterations": 8}},
        {"name": "f", "type": "fast_mcts", "thinking_time_ms": 20, "params": fast_params or {}}],
        "num_games": 3, "seed": 5, "seat_policy": "round_robin", "output_root": str(tmp_path),
        "snapshots": {"enabled": snapshots, "checkpoints": [0, 8, 40, 64]}})


def _fake_record(game_index, game_seed, seat_assignment):
    return {"game_index": game_index, "game_seed": game_seed, "seat_assignment": seat_assignment, "final_scores": {},
            "winner_ids": [], "winner_agents": [], "is_tie": False, "moves_made": 0, "error": None,
            "agent_move_stats": {}}


def test_run_experiment_routes_snapshot_runs(tmp_path, monkeypatch):
    """With snapshots on, a batchable mixed seating goes to run_games_batched with a list for
    its rows (the parent sent it to the host loop); a seating the batched driver cannot play
    still takes run_single_game; and with snapshots off no list is passed."""
    from reinforcementlearning_blokus_amd.arena import runner
    calls = {"batched": [], "single": 0}

    def fake_batched(run_config, game_indices, *, run_id, device, snapshot_rows=None):
        calls["batched"].append(snapshot_rows)
        out = []
        for gi in game_indices:
            gs = game_seed_from_run_seed(run_config.seed, gi)
            out.append(_fake_record(gi, gs, seat_assignment_for_game(run_config.agent_names, gi, gs,
                                                                     run_config.seat_policy)))
        return out

    def fake_single(*, game_index, game_seed, seat_assignment, **k):
        calls["single"] += 1
        assert "snapshot_batch" in k
        return _fake_record(game_index, game_seed, seat_assignment)

    monkeypatch.setattr(runner, "run_games_batched", fake_batched)
    monkeypatch.setattr(runner, "run_single_game", fake_single)
    monkeypatch.setattr(runner, "compute_summary", lambda records, **k: {"completed_games": len(records)})
    monkeypatch.setattr(runner.SnapshotBatch, "flush", lambda self, rows: None)  # (no captures: no launch)
    cfg = _config(tmp_path / "a")
    seats = seat_assignment_for_game(cfg.agent_names, 0, game_seed_from_run_seed(5, 0), "round_robin")
    assert runner._batchable(cfg, seats) and cfg.snapshots.enabled
    runner.run_experiment(cfg)
    assert calls["single"] == 0 and len(calls["batched"]) == 1
    assert isinstance(calls["batched"][0], list)
    # a wall-clock FastMCTS budget is not batchable: the host loop, as before
    calls["batched"].clear()
    runner.run_experiment(_config(tmp_path / "b", {"deterministic_time_budget": False}))
    assert calls["single"] == 3 and calls["batched"] == []
    # snapshots off: batched as before, and nobody asks for rows
    runner.run_experiment(_config(tmp_path / "c", snapshots=False))
    assert calls["single"] == 3 and calls["batched"] == [None]


def test_host_staged_rounds_never_return_records_without_rows(tmp_path, monkeypatch):
    """run_games_batched asked for rows with device_driver=False plays the games through
    run_single_game with one SnapshotBatch (the host-staged rounds do not capture)."""
    from reinforcementlearning_blokus_amd.arena import runner
    seen = []

    def fake_single(*, game_index, game_seed, seat_assignment, snapshot_batch=None, **k):
        seen.append(snapshot_batch)
        return _fake_record(game_index, game_seed, seat_assignment)

    flushed = []
    monkeypatch.setattr(runner, "run_single_game", fake_single)
    monkeypatch.setattr(runner.SnapshotBatch, "flush", lambda self, rows: flushed.append(rows))
    rows = []
    recs = runner.run_games_batched(_config(tmp_path), [0, 1], run_id="x", device_driver=False, snapshot_rows=rows)
    assert [r["game_index"] for r in recs] == [0, 1]
    assert len(seen) == 2 and seen[0] is seen[1] and isinstance(seen[0], runner.SnapshotBatch)
    assert flushed == [rows] and flushed[0] is rows


def test_arena_step_checks_the_snap_tensors():
    """BlokusGPU.arena_step validates a SnapSlots before anything reaches the library (the
    checks need tensors, not a GPU: CPU tensors are rejected by name)."""
    torch = pytest.importorskip("torch")
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU, SnapSlots
    g = BlokusGPU.__new__(BlokusGPU)  # no handle: the checks come first
    g.device = 0
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt)  # noqa: E731
    args = (z(2, 256), z(2, 2080), z(2), z(2, 16, dt=torch.int32), z(2), z(2, dt=torch.int32), z(2, 32), z(2, 16))
    with pytest.raises(ValueError, match="snap.plies"):
        g.arena_step(*args, snap=SnapSlots([], z(2, 0, 256), z(2, 0, 2080), z(2, 0, dt=torch.int32)))
    with pytest.raises(ValueError, match="snap.plies"):
        g.arena_step(*args, snap=SnapSlots([8, 2], z(2, 2, 256), z(2, 2, 2080), z(2, 2, dt=torch.int32)))
    with pytest.raises(ValueError, match="snap.plies"):
        g.arena_step(*args, snap=SnapSlots([0, 8], z(2, 2, 256), z(2, 2, 2080), z(2, 2, dt=torch.int32)))
    with pytest.raises(ValueError, match="snap.states"):
        g.arena_step(*args, snap=SnapSlots([2, 8], z(2, 2, 256), z(2, 2, 2080), z(2, 2, dt=torch.int32)))
