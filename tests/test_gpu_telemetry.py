"""bk_telemetry (k_telemetry) against tests/golden/telemetry.json, recorded from the
reference by tools/gen_telemetry_fixtures.py: every integer of every record, the
effective-frontier sum bit for bit, the seeded shuffle's picks and the move counts after
them in generation order, for the 56 golden positions plus the fixture's own late-game
ones in ONE launch; then the k = 8 subset, small launches, the device path, the Python
module and the BlokusGame hook.  All comparisons are exact.
"""
import faulthandler
import random

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from tests.conftest import load_golden
from tests.helpers import POS, engine_board, fset_of

pytestmark = pytest.mark.gpu

FIX = load_golden("telemetry.json")
KEYS = FIX["metric_keys"]
NAMES = ("RED", "BLUE", "YELLOW", "GREEN")
INT_FIELDS = ("mobility", "anchor_max", "frontier_size", "frontier_components", "quadrants", "center_dist",
              "dead_self", "dead_opp")
STEP_LIMIT_S = 120  # a launch here takes milliseconds; a hung one ends the run instead of stalling it


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def source(rec):
    """The positions.json-style record (log + current player) a fixture entry rebuilds from."""
    return rec if rec["index"] is None else POS[rec["index"]]


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


@pytest.fixture(scope="module")
def packed():
    """(boards, states, sets) of every fixture position, in fixture order."""
    from reinforcementlearning_blokus_amd.engine.board import pack_states
    boards = [engine_board(source(r)) for r in FIX["positions"]]
    sets = np.array([fset_of(source(r)) for r in FIX["positions"]], dtype=N.FSET_DTYPE)
    return boards, pack_states(boards), sets


@pytest.fixture(scope="module")
def fast(gpu, packed):
    """The one launch over all positions, k = 3 (shared, never modified)."""
    _, states, sets = packed
    out = gpu.telemetry(states, sets, k_samples=3, stability=True)
    assert gpu.last_kernel() == "k_telemetry" and gpu.last_kernel_ms() > 0.0
    assert out.shape == (len(states), 4) and out.dtype == N.PLAYER_METRICS_DTYPE
    return out


def check_record(got, ints, want_eff, where, samples=True):
    for k in INT_FIELDS:
        assert int(got[k]) == ints[k], (where, k, int(got[k]), ints[k])
    assert got["piece_count"].tolist() == ints["piece_count"], (where, "piece_count")
    assert float(got["effective_frontier"]) == want_eff, (where, float(got["effective_frontier"]).hex(),
                                                           want_eff.hex())
    assert int(got["status"]) == 0, (where, "status", int(got["status"]))
    n = len(ints["sample_index"]) if samples else 0
    assert int(got["n_samples"]) == n, (where, "n_samples")
    assert got["sample_index"][:n].tolist() == (ints["sample_index"] if samples else []), (where, "sample_index")
    assert got["sample_mobility"][:n].tolist() == (ints["sample_mobility"] if samples else []), (where, "after")
    assert not got["sample_index"][n:].any() and not got["sample_mobility"][n:].any(), (where, "unused samples")
    assert int(got["rng_draws"]) == (ints["rng_draws"] if samples else 0), (where, "rng_draws")


def eff_of(mode, name):
    return mode["metrics"][name][KEYS.index("effectiveFrontier")]


def test_all_positions_in_one_launch(fast):
    for i, rec in enumerate(FIX["positions"]):
        for p, name in enumerate(NAMES):
            check_record(fast[i, p], rec["fast"]["ints"][p], eff_of(rec["fast"], name),
                         (rec["num_moves"], rec["seed"], name))


def test_k8_subset(gpu, packed):
    _, states, sets = packed
    idx = [i for i, r in enumerate(FIX["positions"]) if "k8" in r]
    assert len(idx) >= 7
    out = gpu.telemetry(states[idx], sets[idx], k_samples=8)
    for j, i in enumerate(idx):
        rec = FIX["positions"][i]
        assert rec["k8"]["k"] == 8
        for p, name in enumerate(NAMES):
            check_record(out[j, p], rec["k8"]["ints"][p], eff_of(rec["k8"], name),
                         (rec["num_moves"], rec["seed"], name, "k8"))


def test_small_launches_equal_the_big_one(gpu, packed, fast):
    _, states, sets = packed
    empty = [i for i, r in enumerate(FIX["positions"]) if r["num_moves"] == 0][:1]
    five = [3, 17, 30, 44, len(states) - 1]
    for idx in (empty, five):
        out = gpu.telemetry(states[idx], sets[idx], k_samples=3)
        assert out.tobytes() == fast[idx].tobytes(), idx
    none = gpu.telemetry(states[:0], sets[:0])
    assert none.shape == (0, 4)


def test_without_stability(gpu, packed, fast):
    _, states, sets = packed
    out = gpu.telemetry(states, sets, k_samples=3, stability=False)
    for k in ("n_samples", "status", "sample_index", "sample_mobility", "rng_draws"):
        assert not out[k].any(), k
    for k in INT_FIELDS + ("piece_count", "effective_frontier"):
        assert np.array_equal(out[k], fast[k]), k


def test_device_path_equals_host_path(gpu, packed, fast):
    import torch
    _, states, sets = packed
    dev = torch.device("cuda", 0)
    st = torch.from_numpy(states.view(np.uint8).reshape(-1, 256).copy()).to(dev)
    fs = torch.from_numpy(sets.view(np.uint8).reshape(-1, N.FSET_DTYPE.itemsize).copy()).to(dev)
    out = gpu.telemetry(st, fs, k_samples=3)
    gpu.synchronize()
    torch.cuda.synchronize()
    assert out.shape == (len(states), 4, N.PLAYER_METRICS_DTYPE.itemsize)
    assert out.cpu().numpy().tobytes() == fast.tobytes()


def test_shuffle_picks_equal_cpython(fast):
    """No reference needed: sample_index is the first k of random.Random(42)'s shuffles of
    range(n_q), chained over the opponents that have moves, in Player order."""
    lengths = set()
    for i in range(fast.shape[0]):
        mob = [int(fast[i, p]["mobility"]) for p in range(4)]
        for p in range(4):
            want = []
            if mob[p] > 0:
                rng = random.Random(42)
                for q in range(4):
                    if q == p or mob[q] == 0:
                        continue
                    order = list(range(mob[q]))
                    rng.shuffle(order)
                    want += order[:3]
                    lengths.add(mob[q])
            n = int(fast[i, p]["n_samples"])
            assert n == len(want) and fast[i, p]["sample_index"][:n].tolist() == want, (i, p, mob)
    assert min(lengths) < 3 and max(lengths) > 512  # lists shorter than k and long ones were shuffled


def test_collect_all_player_metrics_equals_the_reference(packed):
    from reinforcementlearning_blokus_amd.engine import telemetry as T
    from reinforcementlearning_blokus_amd.engine.move_generator import get_shared_generator
    boards, _, _ = packed
    mg = get_shared_generator()
    early = next(i for i, r in enumerate(FIX["positions"]) if r["num_moves"] == 4)
    middle = next(i for i, r in enumerate(FIX["positions"]) if r["num_moves"] == 24)
    stuck = next(i for i, r in enumerate(FIX["positions"])
                 if any(x["mobility"] == 0 for x in r["fast"]["ints"]) and any(x["mobility"] > 0 for x in r["fast"]["ints"]))
    for i in (early, middle, stuck):
        rec = FIX["positions"][i]
        want = {name: dict(zip(KEYS, rec["fast"]["metrics"][name])) for name in NAMES}
        got = T.collect_all_player_metrics(boards[i], mg)
        assert got == want, (rec["num_moves"], rec["seed"])
        assert all(type(v) is float for m in got.values() for v in m.values())
    k8 = next(i for i, r in enumerate(FIX["positions"]) if "k8" in r and r["num_moves"] >= 16)
    want = {name: dict(zip(KEYS, FIX["positions"][k8]["k8"]["metrics"][name])) for name in NAMES}
    assert T.collect_all_player_metrics(boards[k8], mg, fast_mode=False) == want
    many = T.collect_many([boards[early], boards[stuck]], move_generator=mg)
    assert many[1] == {name: dict(zip(KEYS, FIX["positions"][stuck]["fast"]["metrics"][name])) for name in NAMES}
    # without a generator: the reference's fallbacks, the board scans unchanged
    plain = T.collect_all_player_metrics(boards[middle])
    ref = FIX["positions"][middle]["fast"]
    for p, name in enumerate(NAMES):
        assert plain[name]["mobility"] == 2.0 * ref["ints"][p]["frontier_size"]
        assert plain[name]["effectiveFrontier"] == eff_of(ref, name)
        assert plain[name]["deadSpaceNearSelf"] == float(ref["ints"][p]["dead_self"])
    from reinforcementlearning_blokus_amd.engine.board import Player
    one = T.compute_player_metrics(boards[middle], Player.YELLOW, mg)
    assert "deadSpace" not in one and one["mobility"] == float(ref["ints"][2]["mobility"])


def test_game_hook_is_opt_in():
    from reinforcementlearning_blokus_amd.engine.game import BlokusGame
    rng = random.Random(3)

    def play(n):
        game = BlokusGame()
        for _ in range(n):
            assert game.make_move(rng.choice(game.get_legal_moves()))
        return game.game_history

    assert BlokusGame.telemetry_backend is None
    assert all("telemetry" not in e for e in play(2))
    BlokusGame.telemetry_backend = "gpu"
    try:
        history = play(6)
    finally:
        BlokusGame.telemetry_backend = None
    assert len(history) == 6
    for n, e in enumerate(history):
        tel = e["telemetry"]
        before = {x["playerId"]: x["metrics"] for x in tel["before"]}
        after = {x["playerId"]: x["metrics"] for x in tel["after"]}
        mover = e["player_to_move"]
        assert tel["ply"] == n + 1 and tel["moverId"] == mover and list(before) == list(after) == list(NAMES)
        a = e["action"]
        assert tel["moveId"] == f"{a['piece_id']}-{a['orientation']}-{a['anchor_row']}-{a['anchor_col']}"
        assert tel["deltaSelf"] == {k: after[mover][k] - before[mover][k] for k in after[mover]}
        assert set(tel["deltaOppByPlayer"]) == set(NAMES) - {mover}
        assert tel["winProxyDelta"] == tel["deltaAdvantage"]["winProxy"]
        if n:  # a move's "before" is the previous move's "after"
            prev = {x["playerId"]: x["metrics"] for x in history[n - 1]["telemetry"]["after"]}
            assert before == prev


def test_input_errors(gpu, packed):
    import ctypes as C
    _, states, sets = packed
    h, L = gpu.handle, N.load()
    out = np.zeros((1, 4), dtype=N.PLAYER_METRICS_DTYPE)
    st, fs = states[:1].ctypes.data, sets[:1].ctypes.data

    def call(k, flags, outp, n=1):
        cfg = N.BkTelemetryCfg(k, flags)
        return L.bk_telemetry(h.ptr, C.c_void_p(st), C.c_void_p(fs), n, C.byref(cfg), C.c_void_p(outp), N.MEM_HOST)

    assert call(0, 1, out.ctypes.data) == N.EINVAL and "k_samples" in h.error()
    assert call(9, 1, out.ctypes.data) == N.EINVAL
    assert call(3, 2, out.ctypes.data) == N.EINVAL and "flags" in h.error()
    assert call(3, 1, 0) == N.EINVAL
    assert call(3, 1, out.ctypes.data, n=-1) == N.EINVAL
    assert L.bk_telemetry(h.ptr, C.c_void_p(st), C.c_void_p(fs), 1, None, C.c_void_p(out.ctypes.data),
                          N.MEM_HOST) == N.EINVAL
    assert call(3, 1, out.ctypes.data, n=0) == N.OK
    assert not out.view(np.uint8).any()  # none of the rejected calls wrote anything
    assert call(3, 1, out.ctypes.data) == N.OK and int(out[0, 0]["mobility"]) > 0
