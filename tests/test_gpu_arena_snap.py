"""Snapshot capture inside the batched arena step (bk_arena_step_snap, k_rollout_fr_hs):
the slots against SEM_ADVANCE replays of the same games (the comparator run_games_gpu uses,
pinned to the reference by tests/test_gpu_snapshot.py), across steps with skipped games and
forced placements at every ply, and the rows of run_games_batched / run_experiment against
the reference's fixture and against the host game loop.  All comparisons are exact."""
import csv
import ctypes as C
import faulthandler

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ARENA = load_golden("arena_snapshots.json")
STEP_LIMIT_S = 300  # a hung launch ends the run instead of stalling it


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


def _run_config(config):
    from reinforcementlearning_blokus_amd.arena.config import RunConfig
    return RunConfig.from_dict(config)


def _seats(rc, gi):
    from reinforcementlearning_blokus_amd.arena.config import game_seed_from_run_seed, seat_assignment_for_game
    gs = game_seed_from_run_seed(rc.seed, gi)
    return gs, seat_assignment_for_game(rc.agent_names, gi, gs, rc.seat_policy)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _fresh(n, cursors):
    """n games at the empty board with Board()'s tables and the given seat cursors."""
    from reinforcementlearning_blokus_amd.gpu import empty_state
    return (_up(np.repeat(empty_state(), n).view(np.uint8).reshape(n, 256)),
            _up(N.fset_new(n).view(np.uint8).reshape(n, -1)), _up(cursors.view(np.int32).reshape(n, 16)))


def _live(fs):
    """bk_fset records with the slots past each table's mask zeroed: those are never written
    or read (copy_fset_table copies slots 0..mask), so they hold whatever the buffer held."""
    fs = np.array(fs, dtype=N.FSET_DTYPE).copy().reshape(-1)
    for i in range(len(fs)):
        for q in range(4):
            fs["key"][i, q, int(fs["mask"][i, q]) + 1:] = 0
    return fs


# ------------------------------------------------------------------ 1. slots equal replays

def test_slots_equal_advance_replays(gpu):
    import torch

    from reinforcementlearning_blokus_amd.arena.config import agent_seed
    from reinforcementlearning_blokus_amd.gpu import SnapSlots, empty_state
    rc = _run_config(ARENA["random"]["config"])
    n, cps = 4, [1, 2, 8, 40, 64, 84]
    seeds = np.zeros((n, 4), dtype=np.uint32)
    for gi in range(n):
        _, st = _seats(rc, gi)
        seeds[gi] = [agent_seed(rc.seed, gi, st[str(p + 1)]) for p in range(4)]
    cursors = N.mt_cursors(seeds.reshape(-1).tolist()).reshape(n, 16)  # the streams compat_seeds give
    dev = torch.device("cuda", 0)
    zeros = _up(np.zeros(n, np.uint8))
    forced = torch.full((n,), -1, dtype=torch.int32, device=dev)

    def play(snap):
        st, fs, rs = _fresh(n, cursors)
        out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        stop = torch.zeros((n, N.STOP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        gpu.arena_step(st, fs, zeros, rs, zeros, forced, out, stop, max_turns=rc.max_turns, snap=snap)
        torch.cuda.synchronize()
        gpu.synchronize()
        return [t.cpu().numpy() for t in (st, fs, rs, out)]

    plain = play(None)
    assert gpu.last_kernel() == "k_rollout_fr_h"
    slots = SnapSlots.allocate(n, cps)
    assert slots.plies == cps and slots.states.shape == (n, 6, 256) and int(slots.turn.max()) == -1
    snap = play(slots)
    assert gpu.last_kernel() == "k_rollout_fr_hs"
    for a, b, name in zip(plain, snap, ("states", "sets", "rng", "results")):  # capturing changes nothing else
        assert np.array_equal(a, b), name
    res = snap[3].view(N.RESULT_DTYPE).reshape(n)
    assert not res["status"].any()
    s_st = slots.states.cpu().numpy().view(N.STATE_DTYPE).reshape(n, 6)
    s_fs = slots.sets.cpu().numpy().view(N.FSET_DTYPE).reshape(n, 6)
    s_turn = slots.turn.cpu().numpy()
    unhit = 0
    for k, c in enumerate(cps):
        r_st, r_fs, r_res = gpu.rollout_frontier(empty_state(), N.fset_new(1), n, semantics=N.SEM_ADVANCE,
                                                 rng=N.RNG_NUMPY_MT, compat_seeds=seeds, max_plies=c,
                                                 root_index=np.zeros(n, dtype=np.int32), with_results=True)
        assert not r_res["status"].any()
        for i in range(n):
            if int(r_st["move_count"][i]) != c:  # the game ended before its c-th placement
                assert int(s_turn[i, k]) == -1, (i, c)
                assert not s_st[i, k].tobytes().strip(b"\0") and not s_fs[i, k].tobytes().strip(b"\0")
                unhit += 1
                continue
            assert int(s_turn[i, k]) == int(r_res["turns"][i]), (i, c)
            assert s_st[i, k].tobytes() == r_st[i].tobytes(), (i, c)
            assert _live(s_fs[i, k]).tobytes() == _live(r_fs[i]).tobytes(), (i, c)
    final = snap[0].view(N.STATE_DTYPE).reshape(n)
    assert int(final["move_count"][1]) == 56  # fixture game 1: plies 64 and 84 unhit
    assert (s_turn[1] >= 0).tolist() == [True, True, True, True, False, False]
    assert unhit >= n  # nobody places 84 pieces


# ------------------------------------------------------------------ 2. steps, SKIP, every ply

def test_across_steps_skip_and_every_ply(gpu):
    import torch

    from reinforcementlearning_blokus_amd.gpu import SnapSlots
    n, stop_seat = 3, 1
    dev = torch.device("cuda", 0)
    cursors = np.stack([N.mt_cursors([7000 + 4 * i + p for p in range(4)]).reshape(-1) for i in range(n)])
    st, fs, rs = _fresh(n, cursors)
    masks = _up(np.full(n, 0x01 | (16 << stop_seat), np.uint8))  # seat 0 heuristic, seat 1 stops, 2-3 random
    quick = _up(np.zeros(n, np.uint8))
    out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    stop = torch.zeros((n, N.STOP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    slots = SnapSlots.allocate(n, range(1, 85))
    assert len(slots.plies) == 84
    forced = np.full(n, -1, np.int32)
    done = np.zeros(n, bool)
    skipped_steps = 0
    for step in range(48):
        hold = step in (3, 4) and not done[2]  # game 2 sits out two steps (its search "in flight")
        send = forced.copy()
        if hold:
            send[2] = N.FORCE_SKIP
            before = [t[2].clone() for t in (slots.states, slots.sets, slots.turn, st, fs, rs)]
        gpu.arena_step(st, fs, masks, rs, quick, _up(send), out, stop, max_turns=2500, snap=slots)
        torch.cuda.synchronize()
        if hold:
            skipped_steps += 1
            for b, t in zip(before, (slots.states, slots.sets, slots.turn, st, fs, rs)):
                assert torch.equal(b, t[2])
            assert int(before[2].max()) >= 0  # it had slots to lose
        res = out.cpu().numpy().view(N.RESULT_DTYPE).reshape(n)
        for i in range(n):
            if done[i] or send[i] == N.FORCE_SKIP:
                continue
            status = int(res["status"][i])
            assert not status & ~(N.STATUS_STOP | N.STATUS_UNCERT), (step, i, status)
            if status & N.STATUS_STOP:
                forced[i] = N.FORCE_INDEX | 0  # the stop seat plays the first move of its list
            else:
                done[i], forced[i] = True, N.FORCE_SKIP  # finished: leave it alone from here on
        if done.all():
            break
    gpu.synchronize()
    assert done.all() and skipped_steps == 2
    s_st = slots.states.cpu().numpy().view(N.STATE_DTYPE).reshape(n, 84)
    s_turn = slots.turn.cpu().numpy()
    final = st.cpu().numpy().view(N.STATE_DTYPE).reshape(n)
    forced_captures = 0
    for i in range(n):
        made = int(final["move_count"][i])
        assert 8 < made < 84
        assert (s_turn[i] >= 0).tolist() == [k < made for k in range(84)]  # every ply played, none after
        assert (np.diff(s_turn[i, :made]) > 0).all() and int(s_turn[i, 0]) == 1
        prev_used, prev_planes = np.zeros(4, np.uint32), np.zeros((4, 7), np.uint64)
        for k in range(made):
            s = s_st[i, k]
            assert int(s["move_count"]) == slots.plies[k] == k + 1
            changed = [p for p in range(4) if int(s["used"][p]) != int(prev_used[p])]
            assert len(changed) == 1, (i, k, changed)  # one piece of one player
            p = changed[0]
            new_bits = int(s["used"][p]) ^ int(prev_used[p])
            assert bin(new_bits).count("1") == 1 and not new_bits & int(prev_used[p])
            for q in range(4):
                if q != p:
                    assert np.array_equal(s["planes"][q], prev_planes[q]), (i, k, q)
            added = sum(bin(int(a) & ~int(b)).count("1") for a, b in zip(s["planes"][p], prev_planes[p]))
            lost = sum(bin(int(b) & ~int(a)).count("1") for a, b in zip(s["planes"][p], prev_planes[p]))
            assert 1 <= added <= 5 and lost == 0
            forced_captures += p == stop_seat  # the stop seat only ever places forced moves
            prev_used, prev_planes = s["used"].copy(), s["planes"].copy()
        assert s_st[i, made - 1]["planes"].tobytes() == final["planes"][i].tobytes()
    assert forced_captures >= n  # forced placements are captured like any other


# ------------------------------------------------------------------ 3. heuristic seat, reference

def test_heuristic_seat_rows_equal_the_reference():
    from reinforcementlearning_blokus_amd.arena.runner import run_games_batched
    rc = _run_config(ARENA["heuristic"]["config"])
    rows = []
    recs = run_games_batched(rc, [0], run_id="fx", snapshot_rows=rows)
    game = ARENA["heuristic"]["games"][0]
    want = [dict(zip(game["columns"], row)) for row in game["rows"]]
    assert len(rows) == len(want) and len(want) >= 12
    for got, ref in zip(rows, want):
        assert list(got) == list(ref)
        assert got == ref, (ref["checkpoint_ply"], ref["player_id"],
                            {k: (got[k], ref[k]) for k in ref if got[k] != ref[k]})
        assert all(type(got[k]) is type(ref[k]) for k in ref)
    for k, v in game["record"].items():  # every recorded field (the fixture keeps no timing fields)
        assert recs[0][k] == v, k
    assert recs[0]["snapshot_checkpoints_hit"] == game["record"]["snapshot_checkpoints_hit"] == [0, 8, 40]


# ------------------------------------------------------------------ 4-6. search seats

SEARCH_CONFIG = {
    "agents": [{"name": "m", "type": "mcts", "params": {"iterations": 6, "max_rollout_moves": 3}},
               {"name": "f", "type": "fast_mcts", "thinking_time_ms": 1,
                "params": {"deterministic_time_budget": True, "iterations_per_ms": 20.0}},
               {"name": "h", "type": "heuristic"}, {"name": "r", "type": "random"}],
    "num_games": 2, "seed": 99173, "seat_policy": "round_robin",
    "snapshots": {"enabled": True, "checkpoints": [0, 1, 2, 5, 6, 8, 40, 64]}}
TIMING = ("duration_sec", "agent_move_stats")


@pytest.fixture(scope="module")
def host_loop():
    """run_single_game's records and rows of the two search-seat games (computed once)."""
    from reinforcementlearning_blokus_amd.arena.runner import SnapshotBatch, run_single_game
    rc = _run_config(SEARCH_CONFIG)
    batch, rows, recs = SnapshotBatch(rc), [], []
    for gi in range(2):
        gs, seats = _seats(rc, gi)
        recs.append(run_single_game(run_id="fx", game_index=gi, game_seed=gs, run_config=rc, seat_assignment=seats,
                                    agent_configs={a.name: a for a in rc.agents}, snapshot_batch=batch))
        assert recs[-1]["error"] is None, recs[-1]["error"]
    batch.flush(rows)
    return rc, recs, rows


def _assert_same(rows, recs, host_loop):
    _, h_recs, h_rows = host_loop
    assert len(rows) == len(h_rows) > 0
    for got, ref in zip(rows, h_rows):
        assert list(got) == list(ref)
        assert got == ref, (ref["game_index"], ref["checkpoint_ply"], ref["player_id"],
                            {k: (got[k], ref[k]) for k in ref if got[k] != ref[k]})
    for a, b in zip(recs, h_recs):
        assert sorted(a) == sorted(b)
        for k in a:
            if k not in TIMING:
                assert a[k] == b[k], (a["game_index"], k)


def test_search_seats_equal_the_host_loop(host_loop):
    from reinforcementlearning_blokus_amd.arena.runner import run_games_batched
    rc, h_recs, h_rows = host_loop
    rows = []
    recs = run_games_batched(rc, [0, 1], run_id="fx", snapshot_rows=rows)
    _assert_same(rows, recs, host_loop)
    # the condition on the input: a non-zero checkpoint placed by the MCTS seat and one by the
    # FastMCTS seat.  While nobody has passed (turn_index == ply) ply c is seat (c - 1) % 4 + 1's
    kinds = {a.name: a.type for a in rc.agents}
    placed_by = set()
    for r in h_rows:
        c = r["checkpoint_ply"]
        if c > 0 and r["turn_index"] == c:
            _, seats = _seats(rc, r["game_index"])
            placed_by.add(kinds[seats[str((c - 1) % 4 + 1)]])
    assert {"mcts", "fast_mcts"} <= placed_by, placed_by
    assert all(rec["snapshot_checkpoints_hit"][:6] == [0, 1, 2, 5, 6, 8] for rec in recs)


@pytest.mark.parametrize("options", [{"search_streams": 1}, {"handback": True}, {"pipeline": False}])
def test_driver_options_give_the_same_rows(options, host_loop, monkeypatch):
    from reinforcementlearning_blokus_amd.arena.runner import run_games_batched
    monkeypatch.delenv("BK_ARENA_CAPTURE", raising=False)  # a capture directory turns hand-back off
    rc = host_loop[0]
    rows = []
    recs = run_games_batched(rc, [0, 1], run_id="fx", snapshot_rows=rows, **options)
    if options.get("handback"):  # the case means nothing unless the per-search hand-back path ran
        from reinforcementlearning_blokus_amd.arena import runner
        timeline = dict(runner.LAST_BATCH_PROFILE["timeline"])
        assert timeline["handback"] is True and timeline["handback_games"] >= 1, timeline
    _assert_same(rows, recs, host_loop)


def test_snapshots_off_changes_nothing(host_loop):
    from reinforcementlearning_blokus_amd.arena.runner import run_games_batched
    rc, h_recs, _ = host_loop
    unset = run_games_batched(rc, [0, 1], run_id="fx")  # enabled, but nobody asked for rows
    rows = []
    off = run_games_batched(_run_config(dict(SEARCH_CONFIG, snapshots={"enabled": False})), [0, 1], run_id="fx",
                            snapshot_rows=rows)
    assert rows == []
    for a, b, ref in zip(unset, off, h_recs):
        assert a["snapshot_checkpoints_hit"] == b["snapshot_checkpoints_hit"] == []
        for k in ref:
            if k not in TIMING + ("snapshot_checkpoints_hit",):
                assert a[k] == b[k] == ref[k], k


def test_run_experiment_writes_the_rows(tmp_path, host_loop):
    from reinforcementlearning_blokus_amd.analytics.winprob.features import SNAPSHOT_FEATURE_COLUMNS
    from reinforcementlearning_blokus_amd.arena.runner import run_experiment
    _, _, h_rows = host_loop
    out = run_experiment(_run_config(dict(SEARCH_CONFIG, output_root=str(tmp_path))))
    with open(f"{out['run_dir']}/snapshots.csv", newline="") as fh:
        got = list(csv.DictReader(fh))
    assert len(got) == len(h_rows)
    for g, r in zip(got, h_rows):
        assert g["run_id"] == out["run_id"] and g["game_id"] == f"{out['run_id']}_g{r['game_index']:04d}"
        assert list(g) == list(r)
        assert all(float(g[c]) == r[c] for c in SNAPSHOT_FEATURE_COLUMNS)
        for k in ("game_index", "checkpoint_ply", "ply", "turn_index", "current_player_id", "player_id", "final_score"):
            assert int(g[k]) == r[k], k


# ------------------------------------------------------------------ argument checks, real handle

def test_rejected_calls_say_why_and_launch_nothing(gpu):
    import torch
    d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    base = (d.data_ptr() + 255) & ~255
    cfg = N.BkRolloutCfg(N.SEM_ARENA, N.ORDER_FRONTIER, N.RNG_NUMPY_MT, 2500, 0, 0, 0)
    vp, h, L = C.c_void_p, gpu.handle, N.load()
    gpu.handle.has_moves(base, 1, base + 61440, N.MEM_DEVICE)  # another kernel is now the last one
    gpu.synchronize()
    last = gpu.last_kernel()

    def call(mask=(1 << 8, 0, 0, 0), states=base + 8192, sets=base + 16384, turn=base + 32768, mem=N.MEM_DEVICE):
        plan = N.BkSnapPlan((C.c_uint32 * 4)(*mask), states, sets, turn)
        return L.bk_arena_step_snap(h.ptr, vp(base), vp(base + 1024), 1, C.byref(cfg), vp(base + 4096), vp(0), vp(0),
                                    vp(base + 4352), vp(base + 4608), vp(0), C.byref(plan), mem)

    assert call(mem=N.MEM_HOST) == N.EINVAL and "BK_MEM_DEVICE" in h.error()
    assert call(mask=(0, 0, 0, 0)) == N.EINVAL and "empty" in h.error()
    assert call(mask=(3, 0, 0, 0)) == N.EINVAL and "ply 0" in h.error()
    assert call(sets=base + 16392) == N.EINVAL and "aligned" in h.error()
    assert call(turn=0) == N.EINVAL and call(states=0) == N.EINVAL
    assert gpu.last_kernel() == last  # none of these launched


# ------------------------------------------------------------------ all-random: one launch or replays

def test_all_random_single_launch_equals_the_replays():
    """run_games_gpu with snapshots on plays one bk_arena_step_snap launch; its earlier route
    (snapshot_replay: one SEM_ADVANCE replay per checkpoint) gives the same rows and records."""
    from reinforcementlearning_blokus_amd.arena.runner import run_games_gpu
    rc = _run_config(ARENA["random"]["config"])
    one, replay = [], []
    recs_one = run_games_gpu(rc, [0, 1, 2], run_id="fx", snapshot_rows=one)
    recs_replay = run_games_gpu(rc, [0, 1, 2], run_id="fx", snapshot_rows=replay, snapshot_replay=True)
    assert one == replay and len(one) >= 16 + 12
    assert all(type(a[k]) is type(b[k]) for a, b in zip(one, replay) for k in a)
    for a, b in zip(recs_one, recs_replay):
        for k in a:
            if k not in TIMING:
                assert a[k] == b[k], (a["game_index"], k)
