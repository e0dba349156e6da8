"""bk_snapshot_features (k_snapshot) against tests/golden/winprob_features.json and
tests/golden/arena_snapshots.json, both recorded from the reference by
tools/gen_winprob_fixtures.py: every integer of every record and every double of every
row for all fixture positions in ONE launch, small launches, the device path, the
single-output calls, bk_telemetry's counts, the argument checks, the Python module, and
the arena's snapshot rows on its two capturing paths.  All comparisons are exact."""
import base64
import ctypes as C
import faulthandler
import zlib

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

FIX = load_golden("winprob_features.json")
ARENA = load_golden("arena_snapshots.json")
COLUMNS = FIX["columns"]
INT_FIELDS = ("mobility", "frontier_size", "corner_differential", "opponent_adjacency", "deadzone_count",
              "occupied_cells", "own_cells", "center_dist", "used_count", "opp_moves_sum", "move_count", "status",
              "reserved", "turn_index")
STEP_LIMIT_S = 120  # a launch here takes milliseconds; a hung one ends the run instead of stalling it


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


def _decode(text, dtype):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype=dtype).copy()


@pytest.fixture(scope="module")
def packed():
    """(states, sets, turn_index) of every fixture position, in fixture order."""
    states = np.concatenate([_decode(r["state"], N.STATE_DTYPE) for r in FIX["positions"]])
    sets = np.concatenate([_decode(r["sets"], N.FSET_DTYPE) for r in FIX["positions"]])
    turns = np.array([r["turn_index"] for r in FIX["positions"]], dtype=np.int32)
    assert len(states) == len(sets) == len(FIX["positions"])
    return states, sets, turns


def by_max_turns():
    """Fixture indices grouped by max_turns (one launch takes one value)."""
    groups = {}
    for i, r in enumerate(FIX["positions"]):
        groups.setdefault(r["max_turns"], []).append(i)
    return groups


@pytest.fixture(scope="module")
def full(gpu, packed):
    """All positions of each max_turns value in one launch (shared, never modified):
    (records [n, 4], features [n, 4, 34]) in fixture order."""
    states, sets, turns = packed
    rec = np.zeros((len(states), 4), dtype=N.SNAPSHOT_REC_DTYPE)
    feat = np.zeros((len(states), 4, 34))
    groups = by_max_turns()
    assert sorted(groups) == [100, 2500] and len(groups[2500]) >= 40
    for mt, idx in groups.items():
        r, f = gpu.snapshot_features(states[idx], sets[idx], turns[idx], mt)
        assert gpu.last_kernel() == "k_snapshot" and gpu.last_kernel_ms() > 0.0
        assert r.shape == (len(idx), 4) and r.dtype == N.SNAPSHOT_REC_DTYPE and f.shape == (len(idx), 4, 34)
        rec[idx], feat[idx] = r, f
    return rec, feat


def test_all_positions(full):
    rec, feat = full
    for i, fx in enumerate(FIX["positions"]):
        for p in range(4):
            where = (fx["num_moves"], fx["seed"], p)
            ints = fx["ints"][p]
            for k in INT_FIELDS:
                assert int(rec[i, p][k]) == ints[k], (where, k, int(rec[i, p][k]), ints[k])
            assert rec[i, p]["piece_count"].tolist() == ints["piece_count"], where
            assert rec[i, p]["frontier_sizes"].tolist() == ints["frontier_sizes"], where
            got = feat[i, p].tolist()
            for c, g, w in zip(COLUMNS, got, fx["rows"][p]):  # bit-equal to CPython's floats
                assert g == w, (where, c, g.hex(), float(w).hex())


def test_small_launches_equal_the_big_one(gpu, packed, full):
    states, sets, turns = packed
    rec, feat = full
    idx = by_max_turns()[2500]
    for sub in ([idx[0]], [idx[5], idx[17], idx[-1]]):  # one block; a 3-board launch
        r, f = gpu.snapshot_features(states[sub], sets[sub], turns[sub], 2500)
        assert r.tobytes() == rec[sub].tobytes() and f.tobytes() == feat[sub].tobytes(), sub


def test_single_outputs_agree(gpu, packed, full):
    states, sets, turns = packed
    rec, feat = full
    idx = by_max_turns()[100]
    r, none = gpu.snapshot_features(states[idx], sets[idx], turns[idx], 100, features=False)
    assert none is None and r.tobytes() == rec[idx].tobytes()
    none, f = gpu.snapshot_features(states[idx], sets[idx], turns[idx], 100, records=False)
    assert none is None and f.tobytes() == feat[idx].tobytes()
    with pytest.raises(ValueError):
        gpu.snapshot_features(states[idx], sets[idx], turns[idx], 100, records=False, features=False)


def test_device_path_equals_host_path(gpu, packed, full):
    import torch
    states, sets, turns = packed
    rec, feat = full
    idx = by_max_turns()[2500]
    dev = torch.device("cuda", 0)
    st = torch.from_numpy(states[idx].view(np.uint8).reshape(-1, 256).copy()).to(dev)
    fs = torch.from_numpy(sets[idx].view(np.uint8).reshape(-1, N.FSET_DTYPE.itemsize).copy()).to(dev)
    ti = torch.from_numpy(turns[idx].copy()).to(dev)
    r, f = gpu.snapshot_features(st, fs, ti, 2500)
    gpu.synchronize()
    torch.cuda.synchronize()
    assert r.shape == (len(idx), 4, 80) and r.dtype == torch.uint8
    assert f.shape == (len(idx), 4, 34) and f.dtype == torch.float64 and f.is_cuda
    assert r.cpu().numpy().tobytes() == rec[idx].tobytes()
    assert f.cpu().numpy().tobytes() == feat[idx].tobytes()
    with pytest.raises(ValueError):
        gpu.snapshot_features(st, fs, ti.to(torch.int64), 2500)


def test_counts_equal_telemetry(gpu, packed, full):
    states, sets, _ = packed
    rec, _ = full
    tel = gpu.telemetry(states, sets, stability=False)
    for k in ("mobility", "piece_count", "frontier_size", "center_dist"):
        assert np.array_equal(tel[k], rec[k]), k


def test_invalid_tables_and_states_are_flagged(gpu, packed, full):
    states, sets, turns = packed
    i = by_max_turns()[2500][9]
    bad_sets = sets[[i, i]].copy()
    bad_sets["mask"][0, 2] = N.FSET_SLOTS          # a header out of range
    bad_sets["key"][1, 1, 0] = 400                  # a key off the board
    bad_states = states[[i]].copy()
    bad_states["planes"][0, 1] |= bad_states["planes"][0, 0]  # two players on the same cells
    r, _ = gpu.snapshot_features(states[[i, i]], bad_sets, turns[[i, i]], 2500)
    assert (r["status"] == N.SNAP_ST_TABLE).all()
    r, _ = gpu.snapshot_features(bad_states, sets[[i]], turns[[i]], 2500)
    assert (r["status"] == N.SNAP_ST_STATE).all()
    assert not full[0]["status"].any()


def test_input_errors(gpu, packed):
    import torch
    states, sets, turns = packed
    h, L = gpu.handle, N.load()
    rec = np.zeros((1, 4), dtype=N.SNAPSHOT_REC_DTYPE)
    feat = np.zeros((1, 4, 34))
    st, fs, ti = states[:1].ctypes.data, sets[:1].ctypes.data, turns[:1].ctypes.data

    def call(st=st, fs=fs, n=1, ti=ti, max_turns=2500, rec=rec.ctypes.data, feat=feat.ctypes.data, mem=N.MEM_HOST):
        return L.bk_snapshot_features(h.ptr, C.c_void_p(st), C.c_void_p(fs), n, C.c_void_p(ti), max_turns,
                                      C.c_void_p(rec), C.c_void_p(feat), mem)

    gpu.synchronize()
    assert call() == N.OK and gpu.last_kernel() == "k_snapshot"
    good = (rec.copy(), feat.copy())
    assert int(rec[0, 0]["mobility"]) > 0
    rec.view(np.uint8)[:] = 0
    feat[:] = 0.0
    mask = np.zeros(1, np.uint8)
    gpu.handle.has_moves(st, 1, mask.ctypes.data, N.MEM_HOST)  # another kernel is now the last one
    last = gpu.last_kernel()
    assert last != "k_snapshot"
    assert call(st=0) == N.EINVAL
    assert call(fs=0) == N.EINVAL
    assert call(ti=0) == N.EINVAL
    assert call(rec=0, feat=0) == N.EINVAL and "both NULL" in h.error()
    assert call(max_turns=-1) == N.EINVAL and "max_turns" in h.error()
    assert call(n=-1) == N.EINVAL
    assert call(mem=2) == N.EINVAL
    # device pointers: the documented alignments (checked before anything is read)
    d = torch.zeros(8192, dtype=torch.uint8, device="cuda:0")
    base = (d.data_ptr() + 255) & ~255
    dev = dict(st=base, fs=base + 1024, ti=base + 4096, rec=base + 4352, feat=base + 5120, mem=N.MEM_DEVICE)
    for name, off in (("fs", 8), ("st", 4), ("rec", 4), ("feat", 4), ("ti", 2)):
        assert call(**dict(dev, **{name: dev[name] + off})) == N.EINVAL and "aligned" in h.error(), name
    assert call(n=0) == N.OK
    assert call(n=0, **dev) == N.OK
    assert gpu.last_kernel() == last                                  # none of these launched
    assert not rec.view(np.uint8).any() and not feat.any()            # or wrote anything
    assert call() == N.OK and rec.tobytes() == good[0].tobytes() and feat.tobytes() == good[1].tobytes()


def test_python_module_equals_the_reference(full):
    from reinforcementlearning_blokus_amd.analytics import winprob as W
    from reinforcementlearning_blokus_amd.engine.board import Player
    from reinforcementlearning_blokus_amd.engine.move_generator import get_shared_generator
    from tests.helpers import POS, engine_board
    pick = [i for i, r in enumerate(FIX["positions"]) if r["index"] is not None and r["max_turns"] == 2500]
    pick = [pick[0], pick[len(pick) // 2], pick[-1]]
    boards = [engine_board(POS[FIX["positions"][i]["index"]]) for i in pick]
    many = W.snapshot_features_many(boards, [FIX["positions"][i]["turn_index"] for i in pick], 2500)
    for b, i, got in zip(boards, pick, many):
        fx = FIX["positions"][i]
        want = {p.name: dict(zip(COLUMNS, fx["rows"][p.value - 1])) for p in Player}
        assert got == want, (fx["num_moves"], fx["seed"])
        assert all(type(v) is float for row in got.values() for v in row.values())
    b, fx = boards[-1], FIX["positions"][pick[-1]]
    ctx = W.build_snapshot_runtime_context(b, turn_index=fx["turn_index"], max_turns=2500)
    assert (ctx.ply, ctx.turn_index, ctx.deadzone_count) == (b.move_count, fx["turn_index"],
                                                             fx["ints"][0]["deadzone_count"])
    for p in (Player.RED, Player.GREEN):
        one = W.extract_player_snapshot_features(b, player=p, context=ctx, move_generator=get_shared_generator())
        assert W.coerce_feature_dict(one) == dict(zip(COLUMNS, fx["rows"][p.value - 1]))
    assert W.snapshot_features_many([], [], 2500) == []


# ------------------------------------------------------------------------------ arena


def _run_config(config):
    from reinforcementlearning_blokus_amd.arena.config import RunConfig
    return RunConfig.from_dict(config)


def _fixture_rows(games):
    return [dict(zip(g["columns"], row)) for g in games for row in g["rows"]]


def _host_loop(rc, game_indices):
    from reinforcementlearning_blokus_amd.arena.config import game_seed_from_run_seed, seat_assignment_for_game
    from reinforcementlearning_blokus_amd.arena.runner import run_single_game
    rows, recs = [], []
    for gi in game_indices:
        gs = game_seed_from_run_seed(rc.seed, gi)
        seats = seat_assignment_for_game(rc.agent_names, gi, gs, rc.seat_policy)
        recs.append(run_single_game(run_id="fx", game_index=gi, game_seed=gs, run_config=rc, seat_assignment=seats,
                                    agent_configs={a.name: a for a in rc.agents}, snapshot_rows=rows))
    return recs, rows


@pytest.fixture(scope="module")
def random_rows():
    """run_games_gpu's records and snapshot rows of the two all-random fixture games."""
    from reinforcementlearning_blokus_amd.arena.runner import run_games_gpu
    rc = _run_config(ARENA["random"]["config"])
    rows = []
    recs = run_games_gpu(rc, [0, 1], run_id="fx", snapshot_rows=rows)
    return rc, recs, rows


def test_advance_replay_ends_where_the_arena_run_ends(gpu):
    """SEM_ADVANCE with a budget of 84 placements (more than a game can hold) and the
    SEM_ARENA run of the same seeds end in the same positions and tables: the replays to
    the checkpoints are prefixes of the arena's games."""
    from reinforcementlearning_blokus_amd.arena.config import (agent_seed, game_seed_from_run_seed,
                                                               seat_assignment_for_game)
    from reinforcementlearning_blokus_amd.gpu import empty_state
    rc = _run_config(ARENA["random"]["config"])
    n = 16
    seeds = np.zeros((n, 4), dtype=np.uint32)
    for gi in range(n):
        st = seat_assignment_for_game(rc.agent_names, gi, game_seed_from_run_seed(rc.seed, gi), rc.seat_policy)
        seeds[gi] = [agent_seed(rc.seed, gi, st[str(p + 1)]) for p in range(4)]
    kw = dict(rng=N.RNG_NUMPY_MT, compat_seeds=seeds, root_index=np.zeros(n, dtype=np.int32))
    a_st, a_fs, a_res = gpu.rollout_frontier(empty_state(), N.fset_new(1), n, semantics=N.SEM_ARENA, max_plies=2500,
                                             with_states=True, **kw)
    b_st, b_fs, b_res = gpu.rollout_frontier(empty_state(), N.fset_new(1), n, semantics=N.SEM_ADVANCE, max_plies=84,
                                             with_results=True, **kw)
    assert not a_res["status"].any() and not b_res["status"].any()
    for k in ("planes", "used", "first_move", "move_count"):
        assert np.array_equal(a_st[k], b_st[k]), k
    assert (a_st["move_count"] < 84).all() and (a_st["move_count"] > 8).all()
    for k in ("key", "mask", "fill", "used"):
        assert np.array_equal(a_fs[k], b_fs[k]), k
    assert np.array_equal(a_res["scores"], b_res["scores"])


def test_all_random_rows_equal_the_reference(random_rows):
    _, recs, rows = random_rows
    games = ARENA["random"]["games"]
    want = _fixture_rows(games)
    assert len(rows) == len(want) == 16 + 12  # game 1 ends before its 64th placement: no row for it
    for got, ref in zip(rows, want):
        assert list(got) == list(ref)  # the reference's column order
        for k in ref:  # every feature, turn_index, ply, current_player_id, the labels, the metadata
            assert got[k] == ref[k], (ref["game_index"], ref["checkpoint_ply"], ref["player_id"], k, got[k], ref[k])
            assert type(got[k]) is type(ref[k]), k
    for rec, g in zip(recs, games):
        assert rec["snapshot_checkpoints_hit"] == g["record"]["snapshot_checkpoints_hit"]
        for k in ("game_seed", "seat_assignment", "winner_ids", "final_scores", "moves_made", "turn_count", "passes"):
            assert rec[k] == g["record"][k], k


def test_snapshots_off_changes_nothing(random_rows):
    from reinforcementlearning_blokus_amd.arena.runner import run_games_gpu
    rc, recs, _ = random_rows
    off = _run_config(dict(ARENA["random"]["config"], snapshots={"enabled": False}))
    rows = []
    plain = run_games_gpu(off, [0, 1], run_id="fx", snapshot_rows=rows)
    assert rows == []
    unset = run_games_gpu(rc, [0, 1], run_id="fx")  # enabled, but nobody asked for rows
    for a, b, c in zip(plain, unset, recs):
        assert a["snapshot_checkpoints_hit"] == b["snapshot_checkpoints_hit"] == []
        for k in a:
            if k not in ("duration_sec", "agent_move_stats", "snapshot_checkpoints_hit"):
                assert a[k] == b[k] == c[k], k


def test_host_loop_rows_equal_run_games_gpu(random_rows):
    rc, recs, rows = random_rows
    host_recs, host_rows = _host_loop(rc, [0, 1])
    assert host_rows == rows  # two independent routes to the same rows
    for a, b in zip(host_recs, recs):
        assert a["snapshot_checkpoints_hit"] == b["snapshot_checkpoints_hit"] and a["final_scores"] == b["final_scores"]


def test_heuristic_seat_game_equals_the_reference():
    rc = _run_config(ARENA["heuristic"]["config"])
    recs, rows = _host_loop(rc, [0])
    game = ARENA["heuristic"]["games"][0]
    want = _fixture_rows([game])
    assert len(rows) == len(want) and len(want) >= 12
    for got, ref in zip(rows, want):
        assert got == ref, (ref["checkpoint_ply"], ref["player_id"], {k: (got[k], ref[k]) for k in ref if got[k] != ref[k]})
    assert recs[0]["snapshot_checkpoints_hit"] == game["record"]["snapshot_checkpoints_hit"]
    assert recs[0]["final_scores"] == game["record"]["final_scores"]


def test_run_experiment_writes_snapshots_csv(tmp_path, random_rows):
    import csv

    from reinforcementlearning_blokus_amd.arena.runner import run_experiment
    _, _, rows = random_rows
    rc = _run_config(dict(ARENA["random"]["config"], output_root=str(tmp_path / "on")))
    out = run_experiment(rc)
    with open(f"{out['run_dir']}/snapshots.csv", newline="") as fh:
        got = list(csv.DictReader(fh))
    assert len(got) == len(rows)
    for g, r in zip(got, rows):
        assert g["run_id"] == out["run_id"] and g["game_id"] == f"{out['run_id']}_g{r['game_index']:04d}"
        assert list(g) == list(r)
        assert all(float(g[c]) == r[c] for c in COLUMNS) and int(g["turn_index"]) == r["turn_index"]
    import json
    with open(f"{out['run_dir']}/games.jsonl") as fh:
        games = [json.loads(line) for line in fh]
    assert [g["snapshot_checkpoints_hit"] for g in games] == [[0, 8, 40, 64], [0, 8, 40]]
    off = _run_config(dict(ARENA["random"]["config"], output_root=str(tmp_path / "off"), snapshots={"enabled": False}))
    out = run_experiment(off)
    import os
    assert sorted(os.listdir(out["run_dir"])) == ["games.jsonl", "run_config.json", "summary.json"]
