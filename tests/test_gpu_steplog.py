"""bk_step_metrics (k_steplog) against tests/golden/steplog_steps.json and
tests/golden/steplog_game.json, both recorded from the reference by
tools/gen_steplog_fixtures.py: every integer of every record for all fixture steps in ONE
launch, small launches, the device path, bk_snapshot_features' counts, the whole sample game
through StrategyLogger, the drop-in metric functions, and the argument and status paths.
All comparisons are exact."""
import base64
import ctypes as C
import faulthandler
import json
import zlib

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

FIX = load_golden("steplog_steps.json")
GAME = load_golden("steplog_game.json")
CASES = FIX["cases"]
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
    """(before, sets_before, after, sets_after, steps) of every fixture case, in fixture order."""
    before = np.concatenate([_decode(c["before"]["state"], N.STATE_DTYPE) for c in CASES])
    sets_before = np.concatenate([_decode(c["before"]["sets"], N.FSET_DTYPE) for c in CASES])
    after = np.concatenate([_decode(c["after"]["state"], N.STATE_DTYPE) for c in CASES])
    sets_after = np.concatenate([_decode(c["after"]["sets"], N.FSET_DTYPE) for c in CASES])
    steps = np.zeros(len(CASES), dtype=N.STEP_DTYPE)
    for i, c in enumerate(CASES):
        steps[i] = tuple(c["step"]) + ([0, 0, 0],)
    assert len(before) == len(sets_before) == len(after) == len(sets_after) == len(CASES) <= 120
    return before, sets_before, after, sets_after, steps


@pytest.fixture(scope="module")
def full(gpu, packed):
    """All fixture cases in one launch (shared, never modified)."""
    rec = gpu.step_metrics(*packed)
    assert gpu.last_kernel() == "k_steplog" and gpu.last_kernel_ms() > 0.0
    assert rec.shape == (len(CASES),) and rec.dtype == N.STEP_REC_DTYPE
    return rec


def sub(packed, idx):
    return tuple(a[idx] for a in packed)


def index_of(flag):
    """The first case showing a coverage property (recomputed from its integers)."""
    for i, c in enumerate(CASES):
        if flag(c):
            return i
    raise AssertionError("no such case")


def test_all_cases(full):
    for i, c in enumerate(CASES):
        where = (c["num_moves"], c["seed"], c["step"])
        for k in FIX["rec_fields"]:
            got = full[i][k].tolist()
            assert got == c["ints"][k], (where, k, got, c["ints"][k])
    assert not full["status"].any()


def test_small_launches_equal_the_big_one(gpu, packed, full):
    first = index_of(lambda c: c["ints"]["area_before"] == 0 and c["ints"]["dist_to_opp_min"] == 40)
    edge = index_of(lambda c: c["ints"]["area_before"] > 0 and c["step"][3] == 0)
    for idx in ([first], [first, edge, len(CASES) - 1]):  # one block; a 3-step launch
        assert gpu.step_metrics(*sub(packed, idx)).tobytes() == full[idx].tobytes(), idx


def test_device_path_equals_host_path(gpu, packed, full):
    import torch
    dev = torch.device("cuda", 0)
    tensors = [torch.from_numpy(a.view(np.uint8).reshape(len(CASES), -1).copy()).to(dev) for a in packed]
    out = gpu.step_metrics(*tensors)
    gpu.synchronize()
    torch.cuda.synchronize()
    assert out.shape == (len(CASES), 64) and out.dtype == torch.uint8 and out.is_cuda
    assert out.cpu().numpy().tobytes() == full.tobytes()
    with pytest.raises(ValueError):
        gpu.step_metrics(tensors[0], tensors[1], tensors[2], tensors[3], tensors[4][:, :4].contiguous())


def test_counts_equal_snapshot_features(gpu, packed, full):
    before, sets_before, after, sets_after, _ = packed
    turns = np.zeros(len(CASES), dtype=np.int32)
    for states, sets, mob, fr in ((before, sets_before, "moves_before", "frontier_before"),
                                  (after, sets_after, "moves_after", "frontier_after")):
        snap, _ = gpu.snapshot_features(states, sets, turns, 2500, features=False)
        assert not snap["status"].any()
        assert np.array_equal(snap["mobility"], full[mob]), mob
        assert np.array_equal(snap["frontier_sizes"][:, 0, :], full[fr]), fr


# ------------------------------------------------------------------------------ the game


def _strip(path):
    lines = [json.loads(x) for x in open(path)]
    assert all(type(ln.pop("timestamp")) is float for ln in lines)
    return lines


def _replay(logger):
    """The fixture game's actions through this package's BlokusGame, logged as the helper logs."""
    from reinforcementlearning_blokus_amd.engine.board import Player
    from reinforcementlearning_blokus_amd.engine.game import BlokusGame
    from reinforcementlearning_blokus_amd.engine.move_generator import Move
    game = BlokusGame(enable_telemetry=False)
    logger.on_reset(GAME["game_id"], GAME["seed"], {p.value: f"RandomAgent_{p.name}" for p in Player}, {})
    for line in GAME["lines"]:
        player = Player(line["player_id"])
        while game.get_current_player() != player:  # the passes of the recorded game
            game.board._update_current_player()
        before = game.get_board_copy()
        a = line["action"]
        move = Move(a["piece_id"], a["orientation"], a["anchor_row"], a["anchor_col"])
        assert game.make_move(move, player)
        logger.on_step(line["game_id"], line["turn_index"], player.value, before, move, game.board)
    res = game.get_game_result()
    logger.on_game_end(GAME["game_id"], res.scores, res.winner_ids[0] if not res.is_tie else None, len(GAME["lines"]))


def test_the_whole_game(tmp_path):
    from reinforcementlearning_blokus_amd.agents.random_agent import RandomAgent
    from reinforcementlearning_blokus_amd.analytics.logging import StrategyLogger, run_game_with_logging
    from reinforcementlearning_blokus_amd.engine.board import Player
    one = StrategyLogger(str(tmp_path / "one"))
    _replay(one)
    assert _strip(one.steps_path) == GAME["lines"]
    assert _strip(one.results_path) == [GAME["result"]]
    batched = StrategyLogger(str(tmp_path / "batched"), batch_steps=1000)
    _replay(batched)  # one flush, at the end
    assert _strip(batched.steps_path) == _strip(one.steps_path)
    assert _strip(batched.results_path) == [GAME["result"]]
    played = StrategyLogger(str(tmp_path / "played"), batch_steps=64)
    run_game_with_logging(GAME["game_id"], {p: RandomAgent(seed=p.value) for p in Player}, played, seed=GAME["seed"])
    lines = _strip(played.steps_path)
    assert [(ln["player_id"], ln["action"]) for ln in lines] == [(ln["player_id"], ln["action"]) for ln in GAME["lines"]]
    assert lines == GAME["lines"] and _strip(played.results_path) == [GAME["result"]]


def test_the_seven_functions_make_one_launch(monkeypatch):
    from reinforcementlearning_blokus_amd.analytics import metrics as M
    from reinforcementlearning_blokus_amd.engine.board import Board, Player, Position
    from reinforcementlearning_blokus_amd.engine.move_generator import Move, get_shared_generator
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    launches = []
    real = BlokusGPU.step_metrics

    def counted(self, *args):
        launches.append(len(args[-1]))
        return real(self, *args)

    monkeypatch.setattr(BlokusGPU, "step_metrics", counted)
    # the fixture game's first two placements, through this package's Board
    board = Board()
    mg = get_shared_generator()
    inps = []
    for line in GAME["lines"][:2]:
        a = line["action"]
        move = Move(a["piece_id"], a["orientation"], a["anchor_row"], a["anchor_col"])
        before = board.copy()
        cells = move.get_positions(mg.piece_orientations_cache[move.piece_id])
        assert board.place_piece(cells, Player(line["player_id"]), move.piece_id)
        inps.append((M.MetricInput(state=before, move=move, next_state=board.copy(), player_id=line["player_id"],
                                   opponents=[q for q in (1, 2, 3, 4) if q != line["player_id"]],
                                   placed_squares=[(p.row, p.col) for p in cells], precomputed_values={}), line))
    assert isinstance(cells[0], Position)
    for inp, line in inps:
        launches.clear()
        got = {}
        for fn in (M.compute_center_metrics, M.compute_territory_metrics, M.compute_mobility_metrics,
                   M.compute_blocking_metrics, M.compute_corner_metrics, M.compute_proximity_metrics,
                   M.compute_piece_metrics):
            got.update(fn(inp))
        assert launches == [1]
        assert got == line["metrics"] and list(got) == list(line["metrics"])
        assert all(type(got[k]) is type(v) for k, v in line["metrics"].items())
        before, after = M.get_mobility_counts(inp)
        assert launches == [1] and before[line["player_id"]] == line["legal_moves_before"]
    inp, line = inps[1]
    many = M.step_metrics_many([i.state for i, _ in inps], [i.next_state for i, _ in inps],
                               [i.player_id for i, _ in inps], [i.move for i, _ in inps])
    assert many == [ln["metrics"] for _, ln in inps] and launches == [1, 2]
    # caller-supplied counts are honoured
    inp.precomputed_values["mobility_counts_before"] = {1: 1, 2: 8, 3: 1, 4: 1}
    assert M.compute_mobility_metrics(inp)["mobility_me_before"] == 8
    assert M.step_metrics_many([], [], [], []) == []


# ------------------------------------------------------------------------------ arguments, status


def test_input_errors(gpu, packed, full):
    import torch
    h, L = gpu.handle, N.load()
    one = [a[:1].copy() for a in packed]
    out = np.zeros(1, dtype=N.STEP_REC_DTYPE)
    ptr = dict(b=one[0].ctypes.data, sb=one[1].ctypes.data, a=one[2].ctypes.data, sa=one[3].ctypes.data,
               st=one[4].ctypes.data, out=out.ctypes.data)

    def call(n=1, mem=N.MEM_HOST, **kw):
        p = dict(ptr, **kw)
        return L.bk_step_metrics(h.ptr, C.c_void_p(p["b"]), C.c_void_p(p["sb"]), C.c_void_p(p["a"]), C.c_void_p(p["sa"]),
                                 C.c_void_p(p["st"]), n, C.c_void_p(p["out"]), mem)

    gpu.synchronize()
    assert call() == N.OK and gpu.last_kernel() == "k_steplog"
    assert out.tobytes() == full[:1].tobytes()
    out.view(np.uint8)[:] = 0
    mask = np.zeros(1, np.uint8)
    gpu.handle.has_moves(ptr["b"], 1, mask.ctypes.data, N.MEM_HOST)  # another kernel is now the last one
    last = gpu.last_kernel()
    assert last != "k_steplog"
    for name in ptr:
        assert call(**{name: 0}) == N.EINVAL, name
    assert call(n=-1) == N.EINVAL and call(mem=2) == N.EINVAL
    # device pointers: the documented alignments (checked before anything is read)
    d = torch.zeros(16384, dtype=torch.uint8, device="cuda:0")
    base = (d.data_ptr() + 255) & ~255
    dev = dict(b=base, sb=base + 1024, a=base + 4096, sa=base + 5120, st=base + 8192, out=base + 8448)
    for name, off in (("sb", 8), ("sa", 8), ("b", 4), ("a", 4), ("st", 4), ("out", 4)):
        assert call(mem=N.MEM_DEVICE, **dict(dev, **{name: dev[name] + off})) == N.EINVAL, name
        assert "aligned" in h.error(), name
    assert call(n=0) == N.OK
    assert call(n=0, mem=N.MEM_DEVICE, **dev) == N.OK
    assert gpu.last_kernel() == last           # none of these launched
    assert not out.view(np.uint8).any()        # or wrote anything
    assert call() == N.OK and out.tobytes() == full[:1].tobytes()
    with pytest.raises(ValueError, match="whole number"):  # a steps buffer that is no whole number of records
        gpu.step_metrics(one[0], one[1], one[2], one[3], one[4].view(np.uint8)[:7])
    with pytest.raises(ValueError, match="sets_after"):
        gpu.step_metrics(one[0], one[1], one[2], packed[3][:2], one[4])


def test_statuses_are_set_and_raise(gpu, packed, full, tmp_path):
    from reinforcementlearning_blokus_amd.analytics import metrics as M
    before, sets_before, after, sets_after, steps = packed
    i = index_of(lambda c: c["num_moves"] >= 12)
    j = index_of(lambda c: c["num_moves"] >= 12 and c["step"] != CASES[i]["step"])
    want = full[i].copy()

    def run(b=before[[i]], sb=sets_before[[i]], a=after[[i]], sa=sets_after[[i]], st=steps[[i]]):
        return gpu.step_metrics(b, sb, a, sa, st)[0]

    assert run().tobytes() == want.tobytes()
    # an after board that is not before plus the step
    assert run(a=after[[j]], sa=sets_after[[j]])["status"] & N.STEP_ST_MOVE
    assert run(a=before[[i]])["status"] == N.STEP_ST_MOVE                     # nothing was placed
    moved = steps[[i]].copy()
    moved["anchor_col"] = (int(moved["anchor_col"][0]) + 1) % 16
    assert run(st=moved)["status"] & N.STEP_ST_MOVE                            # another anchor
    # a piece already used
    used = before[[i]].copy()
    used["used"][0, CASES[i]["step"][0]] |= 1 << (CASES[i]["step"][1] - 1)
    assert run(b=used)["status"] == N.STEP_ST_MOVE
    # a mover above 3, a piece and an orientation outside the table, a cell off the board
    for field, value in (("mover", 4 + CASES[i]["step"][0]), ("piece_id", 0), ("piece_id", 22), ("orientation", 8)):
        bad = steps[[i]].copy()
        bad[field] = value
        r = run(st=bad)
        assert r["status"] == N.STEP_ST_MOVE, (field, value)
        assert r["moves_before"].tolist() == want["moves_before"].tolist()     # the fields are still written
    off = steps[[i]].copy()
    off["anchor_row"], off["anchor_col"] = 19, 19
    off["piece_id"], off["orientation"] = 21, 0
    assert run(st=off)["status"] & N.STEP_ST_MOVE
    # a table header out of range, on either side; overlapping planes
    for side in ("sb", "sa"):
        bad = (sets_before if side == "sb" else sets_after)[[i]].copy()
        bad["mask"][0, 2] = N.FSET_SLOTS
        assert run(**{side: bad})["status"] == N.STEP_ST_TABLE, side
    both = before[[i]].copy()
    both["planes"][0, 1] |= both["planes"][0, 0]
    assert run(b=both)["status"] & N.STEP_ST_STATE
    assert not full["status"].any()
    # the Python layer raises for every status
    for status in (N.STEP_ST_TABLE, N.STEP_ST_STATE, N.STEP_ST_MOVE):
        with pytest.raises(RuntimeError, match=f"status {status}"):
            M.check_record({"status": status})

    class Flagging:
        def step_metrics(self, *args):
            return gpu.step_metrics(before[[i]], sets_before[[i]], before[[i]], sets_after[[i]], steps[[i]])

    from reinforcementlearning_blokus_amd.analytics.logging import StrategyLogger
    from reinforcementlearning_blokus_amd.engine.board import Board
    from reinforcementlearning_blokus_amd.engine.move_generator import Move
    logger = StrategyLogger(str(tmp_path), engine=Flagging())
    with pytest.raises(RuntimeError, match="turn_index 7"):
        logger.on_step("g", 7, 1, Board(), Move(1, 0, 0, 0), Board())
