"""HeuristicAgent seats with weights of their own on the GPU (k_rollout_fr_hw through
bk_rollout_frontier_w / bk_arena_step_w, and the batched arena on top of them) against the
reference's records (tests/golden/heuristic_weights.json,
tools/gen_heuristic_weights_fixtures.py), against the default-weight kernel
(k_rollout_fr_h) where the sets are the defaults, and against the host game loop.
Tolerance: exact."""
import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from reinforcementlearning_blokus_amd.arena import RunConfig
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
FX = load_golden("heuristic_weights.json")
NAMES = ["A", "B", "C", "D"]
SETS = [N.heur_weight_set(FX["weight_sets"][k]) for k in NAMES]
RECORD_FIELDS = ("seat_assignment", "winner_ids", "winner_agents", "is_tie", "final_scores", "final_ranks",
                 "moves_made", "turn_count", "passes", "invalid_actions", "truncated")


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


@pytest.mark.parametrize("device_driver", [True, False])
@pytest.mark.parametrize("key", ["arena_pure", "arena_mixed"])
def test_batched_arena_matches_reference_records(key, device_driver):
    """A run config whose heuristic agents carry "weights" goes through run_games_batched
    (either driver) and returns the reference's run_single_game records
    (arena_runner.py:423-428, :578-777)."""
    from reinforcementlearning_blokus_amd.arena import runner
    cfg = RunConfig.from_dict(FX[key + "_config"])
    recs = runner.run_games_batched(cfg, [r["game_index"] for r in FX[key]], device_driver=device_driver)
    assert runner.LAST_BATCH_PROFILE["uncertified_heuristic"] == 0
    for got, ref in zip(recs, FX[key]):
        for k in ("seat_assignment", "winner_ids", "final_scores", "moves_made", "turn_count", "passes",
                  "invalid_actions", "is_tie"):
            assert got[k] == ref[k], (ref["game_index"], k)


def _game_launch(order):
    """Launch inputs that replay fixture game order[i] as playout i: per-seat seeds and the
    seat-to-set byte (seat p scores with the set the game gave it)."""
    games = [FX["games"][k] for k in order]
    seeds = np.array([[g["seed"] + p + 1 for p in range(4)] for g in games], np.uint32)
    seat_sets = np.array([sum(NAMES.index(s) << (2 * p) for p, s in enumerate(g["seat_sets"])) for g in games],
                         np.uint8)
    return games, seeds, seat_sets


@pytest.mark.parametrize("n", [1, 4, 65])
def test_full_games_match_reference(gpu, n):
    """Full games of four HeuristicAgents, each seat another weight set, from the empty
    board in one bk_rollout_frontier_w launch: one game, all four, and 65 playouts that
    cycle through the four games -- their seat-to-set maps are the four rotations, so every
    (seat, set) pair is played, neighbouring lanes of a wave disagree on the set at every
    seat, and a second, partial wave exists.  The games cross move 30 (the late tables) and
    end on short lists."""
    from reinforcementlearning_blokus_amd.gpu import empty_state
    games, seeds, seat_sets = _game_launch([i % 4 for i in range(n)])
    for p in range(4):  # among four neighbouring playouts seat p uses every set once
        assert n == 1 or sorted(((seat_sets[:4] >> (2 * p)) & 3).tolist()) == [0, 1, 2, 3]
    res = gpu.rollout_frontier(empty_state(), N.fset_new(1), n, semantics=N.SEM_ARENA, rng=N.RNG_NUMPY_MT,
                               compat_seeds=seeds, root_index=np.zeros(n, np.int32), heuristic_seats=0xF,
                               heur_sets=SETS, seat_sets=seat_sets)
    assert "k_rollout_fr_hw" in gpu.last_kernel()
    for i, (r, g) in enumerate(zip(res, games)):
        plies = sum(1 for t in g["trace"] if t >= 0)
        assert int(r["status"]) == 0, i
        assert [int(x) for x in r["scores"]] == g["scores"], i
        assert [p + 1 for p in range(4) if int(r["winner_mask"]) >> p & 1] == g["winner_ids"], i
        assert (int(r["plies"]), int(r["passes"]), int(r["turns"])) == (plies, g["passes"], g["turns"]), i
        # one random_sample (two 32-bit outputs) per placement: the seats' recorded generator positions
        assert sum(g["rng"][str(p + 1)][0] for p in range(4)) == 2 * plies == int(r["draws"]), i


def _same_tables(a, b):
    """Two arrays of bk_fset records hold the same tables: headers equal, and every slot of
    each table (key[p][0..mask[p]]) equal.  Slots past a table's size are not part of it:
    a record keeps there whatever its slab slot held before."""
    a, b = a.view(N.FSET_DTYPE).reshape(-1), b.view(N.FSET_DTYPE).reshape(-1)
    for k in ("mask", "fill", "used"):
        if not np.array_equal(a[k], b[k]):
            return False
    live = np.arange(N.FSET_SLOTS)[None, None, :] <= a["mask"][:, :, None]
    return np.array_equal(a["key"][live], b["key"][live])


N_ID = 130
ID_SEEDS = (np.arange(N_ID * 4, dtype=np.uint32).reshape(N_ID, 4) * 2654435761 + 20260311).astype(np.uint32)
ID_SETS = ((np.arange(N_ID) * 37 + 11) & 0xFF).astype(np.uint8)  # every lane another seat-to-set byte


def test_default_sets_equal_the_default_kernel_rollout(gpu):
    """bk_rollout_frontier_w with four sets that are all the default weights returns the
    records and final positions of bk_rollout_frontier byte for byte, and the same frontier
    tables slot for slot, on 130 all-heuristic arena games from the empty board; every draw
    of both runs is certified."""
    from reinforcementlearning_blokus_amd.gpu import empty_state
    kw = dict(semantics=N.SEM_ARENA, rng=N.RNG_NUMPY_MT, compat_seeds=ID_SEEDS, root_index=np.zeros(N_ID, np.int32),
              heuristic_seats=0xF, with_states=True)
    st0, fs0, res0 = gpu.rollout_frontier(empty_state(), N.fset_new(1), N_ID, **kw)
    assert "k_rollout_fr_h" in gpu.last_kernel() and "k_rollout_fr_hw" not in gpu.last_kernel()
    st1, fs1, res1 = gpu.rollout_frontier(empty_state(), N.fset_new(1), N_ID, heur_sets=[N.HEUR_DEFAULT_WEIGHTS] * 4,
                                          seat_sets=ID_SETS, **kw)
    assert "k_rollout_fr_hw" in gpu.last_kernel()
    assert not res0["status"].any() and not res1["status"].any()
    assert (res0["plies"] > 40).all()
    assert res0.tobytes() == res1.tobytes()
    assert st0.tobytes() == st1.tobytes() and _same_tables(fs0, fs1)


def _arena_tensors(n, seeds, masks):
    import torch

    from reinforcementlearning_blokus_amd.gpu import empty_state
    dev = torch.device("cuda", 0)
    rng = np.zeros((n, 16), np.uint32)
    rng[:] = N.mt_cursors(seeds.reshape(-1)).reshape(n, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return {"states": up(np.repeat(empty_state(), n).view(np.uint8).reshape(n, 256)),
            "sets": up(np.repeat(N.fset_new(1), n).view(np.uint8).reshape(n, -1)),
            "seat_masks": up(masks), "rng_state": up(rng.view(np.int32)),
            "quick_masks": torch.zeros(n, dtype=torch.uint8, device=dev),
            "forced": torch.full((n,), -1, dtype=torch.int32, device=dev),
            "out": torch.full((n, 32), 0xAB, dtype=torch.uint8, device=dev),
            "stop_out": torch.zeros((n, N.STOP_DTYPE.itemsize), dtype=torch.uint8, device=dev)}


def _step(gpu, t, **kw):
    import torch
    gpu.arena_step(t["states"], t["sets"], t["seat_masks"], t["rng_state"], t["quick_masks"], t["forced"], t["out"],
                   t["stop_out"], **kw)
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in ("states", "sets", "rng_state", "out")}


def test_default_sets_equal_the_default_kernel_arena_step(gpu):
    """The same identity through bk_arena_step / bk_arena_step_w in device memory: results,
    positions, tables and the seats' generator cursors."""
    import torch
    masks = np.full(N_ID, 0xF, np.uint8)
    a = _step(gpu, _arena_tensors(N_ID, ID_SEEDS, masks))
    b = _step(gpu, _arena_tensors(N_ID, ID_SEEDS, masks), heur_sets=[N.HEUR_DEFAULT_WEIGHTS] * 4,
              seat_sets=torch.from_numpy(ID_SETS).to("cuda:0"))
    assert "k_rollout_fr_hw" in gpu.last_kernel()
    res = a["out"].view(N.RESULT_DTYPE).reshape(N_ID)
    assert not res["status"].any() and (res["plies"] > 40).all()
    for k in ("states", "rng_state", "out"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert _same_tables(a["sets"], b["sets"])


def test_batched_equals_host_loop_randomized_seats():
    """8 randomized-seat games of heuristic A, heuristic B, MCTS and FastMCTS: the batched
    driver's records equal the host game loop's (run_single_game), game by game."""
    from reinforcementlearning_blokus_amd.arena.config import game_seed_from_run_seed, seat_assignment_for_game
    from reinforcementlearning_blokus_amd.arena.runner import run_games_batched, run_single_game
    cfg = RunConfig.from_dict({
        "agents": [{"name": "ha", "type": "heuristic", "params": {"weights": FX["weight_sets"]["A"]}},
                   {"name": "hb", "type": "heuristic", "params": {"weights": FX["weight_sets"]["B"]}},
                   {"name": "m", "type": "mcts", "params": {"iterations": 6, "max_rollout_moves": 3}},
                   {"name": "f", "type": "fast_mcts", "params": {"time_limit": 0.005}}],
        "num_games": 8, "seed": 99174, "seat_policy": "randomized"})
    batched = run_games_batched(cfg, range(8))
    agents = {a.name: a for a in cfg.agents}
    for gi, got in enumerate(batched):
        gs = game_seed_from_run_seed(cfg.seed, gi)
        seats = seat_assignment_for_game(cfg.agent_names, gi, gs, cfg.seat_policy)
        ref = run_single_game(run_id="h", game_index=gi, game_seed=gs, run_config=cfg, seat_assignment=seats,
                              agent_configs=agents)
        assert ref["error"] is None, ref["error"]
        for k in RECORD_FIELDS:
            assert got[k] == ref[k], (gi, k)


def test_unknown_set_in_device_memory_is_flagged_and_not_played(gpu):
    """A device-memory seat_sets byte that names set 2 of a two-set plan on a heuristic
    seat: that game is not played (its position, tables and cursors are as they were, its
    result is zero but BK_STATUS_BADSET), bk_synchronize reports it once, and the other 64
    games -- the rest of its wave and the partial second wave -- play as without it.  The
    same index on a seat that does not play the heuristic is ignored."""
    import torch
    n, bad = 65, 7
    masks = np.full(n, 0x7, np.uint8)  # seats 0-2 heuristic, seat 3 random
    seat_sets = ((np.arange(n) * 5) & 0x15).astype(np.uint8) | 0xC0  # sets 0 / 1; seat 3 names set 3: ignored
    seeds = ID_SEEDS[:n]
    sets2 = [SETS[0], SETS[1]]
    good = _step(gpu, _arena_tensors(n, seeds, masks), heur_sets=sets2, seat_sets=torch.from_numpy(seat_sets).to("cuda:0"))
    gpu.synchronize()
    res = good["out"].view(N.RESULT_DTYPE).reshape(n)
    assert not (res["status"].astype(np.int64) & ~N.STATUS_UNCERT).any() and (res["plies"] > 40).all()
    wrong = seat_sets.copy()
    wrong[bad] = 0xC0 | (2 << 2)  # seat 1, a heuristic seat, names set 2
    t = _arena_tensors(n, seeds, masks)
    before = {k: t[k][bad].cpu().numpy().copy() for k in ("states", "sets", "rng_state")}
    got = _step(gpu, t, heur_sets=sets2, seat_sets=torch.from_numpy(wrong).to("cuda:0"))
    with pytest.raises(RuntimeError, match="weight set"):
        gpu.synchronize()
    gpu.synchronize()  # reported once
    flagged = got["out"].view(N.RESULT_DTYPE).reshape(n)[bad]
    assert int(flagged["status"]) == N.STATUS_BADSET
    zero = flagged.copy()
    zero["status"] = 0
    assert not zero.tobytes().strip(b"\0")
    for k in before:
        assert got[k][bad].tobytes() == before[k].tobytes(), k
    keep = np.arange(n) != bad
    for k in ("states", "rng_state", "out"):
        assert got[k][keep].tobytes() == good[k][keep].tobytes(), k
    assert _same_tables(np.ascontiguousarray(got["sets"][keep]), np.ascontiguousarray(good["sets"][keep]))


def test_plan_rules_are_refused_with_their_messages(gpu):
    """The plan's own rules on a live handle, each BK_EINVAL with its message before any
    launch: n_sets outside 1..4, a non-finite weight, S over BK_HEUR_MAX_S, and (host
    memory) a heuristic seat that names a set the plan does not have."""
    from reinforcementlearning_blokus_amd.gpu import empty_state
    seeds = ID_SEEDS[:2]

    def play(sets, seat_sets=0, heuristic_seats=0xF):
        return gpu.rollout_frontier(empty_state(), N.fset_new(1), 2, semantics=N.SEM_ARENA, rng=N.RNG_NUMPY_MT,
                                    compat_seeds=seeds, root_index=np.zeros(2, np.int32),
                                    heuristic_seats=heuristic_seats, heur_sets=sets, seat_sets=seat_sets)

    for sets, msg in (([], "n_sets"), ([(1.0, float("nan"), 0.0, 0.0)], "not finite"),
                      ([(0.0, 0.0, float("inf"), 0.0)], "not finite"), ([(0.0, 6.5, 0.0, 0.0)], "BK_HEUR_MAX_S")):
        with pytest.raises(RuntimeError, match=msg):
            play(sets)
    with pytest.raises(RuntimeError, match="n_sets"):  # five sets: the struct holds four, n_sets says five
        plan_sets = [N.HEUR_DEFAULT_WEIGHTS] * 4
        plan = N.heur_plan(plan_sets)
        plan.n_sets = 5
        cfg = N.BkRolloutCfg(N.SEM_ARENA, N.ORDER_FRONTIER, N.RNG_NUMPY_MT, 2500, 0, 0, 0xF)
        out = np.zeros(2, N.RESULT_DTYPE)
        gpu.handle.rollout_frontier_w(empty_state().ctypes.data, N.fset_new(1).ctypes.data, 1, 0, 2, cfg,
                                      seeds.ctypes.data, out.ctypes.data, 0, 0, plan, N.MEM_HOST)
    with pytest.raises(RuntimeError, match="weight set >= n_sets"):
        play([SETS[0]], seat_sets=np.array([0, 1 << 4], np.uint8))
    # the same byte is fine where seat 2 does not play the heuristic, and S = 128 is on the bound
    res = play([SETS[0], (0.0, 6.4, 0.0, 0.0)], seat_sets=np.array([1, 1 << 4], np.uint8), heuristic_seats=0x3)
    assert not (res["status"].astype(np.int64) & ~N.STATUS_UNCERT).any()
