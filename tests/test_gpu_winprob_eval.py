"""bk_winprob_eval (k_winprob) against its specification, host_probabilities in CPython floats
over bk_snapshot_features' rows of the same launch inputs, and against the reference's recorded
values (tests/golden/winprob_eval.json, tools/gen_winprob_eval_fixtures.py).

pair_logit is compared with ``==``: every step of it is one correctly rounded double operation
on both sides.  prob is compared within 8 ulp: exp is documented to 1 ulp, and one add, one
divide, two adds and one divide follow it.  The reference's values are compared within the
rounding bounds of tests/test_winprob_eval_host.py (sklearn sums in another order)."""
import base64
import ctypes as C
import faulthandler
import json
import math
import zlib

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from reinforcementlearning_blokus_amd.mcts.learned_evaluator import (LearnedWinProbabilityEvaluator, WinProbModel,
                                                                     host_probabilities)
from tests.test_winprob_eval_host import EPS, FIX, check_against_reference, logit_bounds

pytestmark = pytest.mark.gpu


def _decode(text, dtype):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype=dtype).copy()


STEP_LIMIT_S = 120  # a launch here takes milliseconds; a hung one ends the run instead of stalling it
MAX_TURNS = FIX["max_turns"]
MODEL = WinProbModel.from_dict(FIX["model"])
SUBSET = WinProbModel.from_dict(FIX["model_subset"])


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


@pytest.fixture(scope="module")
def packed():
    states = np.concatenate([_decode(r["state"], N.STATE_DTYPE) for r in FIX["positions"]])
    sets = np.concatenate([_decode(r["sets"], N.FSET_DTYPE) for r in FIX["positions"]])
    assert len(states) == len(sets) == 60
    assert states["move_count"].tolist() == [r["move_count"] for r in FIX["positions"]]
    return states, sets


@pytest.fixture(scope="module")
def full(gpu, packed):
    """All 60 positions in one launch (shared, never modified): (prob, pair_logit, rows), rows
    from bk_snapshot_features with the evaluator's context (turn_index = move_count)."""
    states, sets = packed
    prob, logit, status = gpu.winprob_eval(states, sets, None, MAX_TURNS, MODEL, pair_logits=True)
    assert gpu.last_kernel() == "k_winprob" and gpu.last_kernel_ms() > 0.0
    assert prob.shape == (60, 4) and logit.shape == (60, 4, 3) and status.shape == (60,) and not status.any()
    rec, rows = gpu.snapshot_features(states, sets, states["move_count"].astype(np.int32), MAX_TURNS)
    assert not rec["status"].any()
    return prob, logit, rows


def check_against_host(model, prob, logit, rows, where):
    worst = 0.0
    for i in range(len(prob)):
        want_p, want_t = host_probabilities(model, rows[i].tolist(), with_logits=True)
        for p in range(4):
            for j in range(3):
                got = float(logit[i, p, j])
                assert got == want_t[p][j], (where, i, p, j, got.hex(), want_t[p][j].hex())
            ulps = abs(float(prob[i, p]) - want_p[p]) / math.ulp(want_p[p])
            assert ulps <= 8, (where, i, p, float(prob[i, p]).hex(), want_p[p].hex(), ulps)
            worst = max(worst, ulps)
    return worst


def test_all_positions(full):
    prob, logit, rows = full
    for i, r in enumerate(FIX["positions"]):  # the launch's rows are the reference's, bit for bit
        assert rows[i].tolist() == r["rows"], (r["num_moves"], r["seed"])
    worst = check_against_host(MODEL, prob, logit, rows, "full")
    print(f"worst prob difference from the host chain: {worst:.2f} ulp")
    for i, r in enumerate(FIX["positions"]):
        check_against_reference(MODEL, r["rows"], logit[i].tolist(), prob[i].tolist(), r["logit"], r["prob"],
                                (r["num_moves"], r["seed"]))
    assert np.isfinite(prob).all() and (prob > 0).all() and (prob < 1).all()
    assert prob.min() < 0.05 and prob.max() > 0.95
    ply0 = [i for i, r in enumerate(FIX["positions"]) if r["move_count"] == 0]
    assert ply0 and all(len(set(prob[i].tolist())) == 1 for i in ply0)


def test_explicit_turn_index_equals_the_default(gpu, packed, full):
    states, sets = packed
    turns = states["move_count"].astype(np.int32)
    prob, logit, _ = gpu.winprob_eval(states, sets, turns, MAX_TURNS, MODEL, pair_logits=True)
    assert prob.tobytes() == full[0].tobytes() and logit.tobytes() == full[1].tobytes()
    # another turn_index and max_turns reach the rows (the columns cancel in every difference,
    # so the results stay; the chain is still checked on those rows)
    prob, logit, _ = gpu.winprob_eval(states, sets, turns + 7, 100, MODEL, pair_logits=True)
    _, rows = gpu.snapshot_features(states, sets, turns + 7, 100, records=False)
    assert not np.array_equal(rows, full[2])
    check_against_host(MODEL, prob, logit, rows, "turn + 7")


def test_subset_model(gpu, packed, full):
    states, sets = packed
    prob, logit, status = gpu.winprob_eval(states, sets, None, MAX_TURNS, SUBSET, pair_logits=True)
    assert not status.any()
    check_against_host(SUBSET, prob, logit, full[2], "subset")
    for i, r in enumerate(FIX["positions"]):
        check_against_reference(SUBSET, r["rows"], logit[i].tolist(), prob[i].tolist(), None, r["prob_subset"],
                                (r["num_moves"], r["seed"]))


def test_small_launches_and_null_logits(gpu, packed, full):
    states, sets = packed
    for sub in ([0], [5, 17, 59]):  # one block; a 3-board launch
        prob, logit, status = gpu.winprob_eval(states[sub], sets[sub], None, MAX_TURNS, MODEL, pair_logits=True)
        assert prob.tobytes() == full[0][sub].tobytes() and logit.tobytes() == full[1][sub].tobytes(), sub
        assert not status.any()
    prob, none, _ = gpu.winprob_eval(states, sets, None, MAX_TURNS, MODEL)
    assert none is None and prob.tobytes() == full[0].tobytes()


def test_device_path_equals_host_path(gpu, packed, full):
    import torch
    states, sets = packed
    dev = torch.device("cuda", 0)
    st = torch.from_numpy(states.view(np.uint8).reshape(-1, 256).copy()).to(dev)
    fs = torch.from_numpy(sets.view(np.uint8).reshape(-1, N.FSET_DTYPE.itemsize).copy()).to(dev)
    ti = torch.from_numpy(states["move_count"].astype(np.int32)).to(dev)
    for turn in (None, ti):
        prob, logit, status = gpu.winprob_eval(st, fs, turn, MAX_TURNS, MODEL, pair_logits=True)
        gpu.synchronize()
        torch.cuda.synchronize()
        assert prob.is_cuda and prob.dtype == torch.float64 and prob.shape == (60, 4) and logit.shape == (60, 4, 3)
        assert status.dtype == torch.uint8 and not status.cpu().numpy().any()
        assert prob.cpu().numpy().tobytes() == full[0].tobytes()
        assert logit.cpu().numpy().tobytes() == full[1].tobytes()
    prob, none, _ = gpu.winprob_eval(st, fs, None, MAX_TURNS, MODEL)
    torch.cuda.synchronize()
    assert none is None and prob.cpu().numpy().tobytes() == full[0].tobytes()
    with pytest.raises(ValueError):
        gpu.winprob_eval(st, fs, ti.to(torch.int64), MAX_TURNS, MODEL)


def test_model_edge_cases(gpu, packed, full):
    states, sets = packed
    zero = WinProbModel([0.0] * 34, [1.0] * 34, [0.0] * 34, 0.0)
    prob, logit, _ = gpu.winprob_eval(states, sets, None, MAX_TURNS, zero, pair_logits=True)
    assert (prob == 0.5).all() and (logit == 0.0).all()
    big = WinProbModel(MODEL.mean, MODEL.scale, [c * 1e6 for c in MODEL.coef], MODEL.intercept)
    prob, logit, status = gpu.winprob_eval(states, sets, None, MAX_TURNS, big, pair_logits=True)
    assert not status.any() and np.isfinite(prob).all() and np.isfinite(logit).all()
    assert (prob >= 0.0).all() and (prob <= 1.0).all() and (prob == 0.0).any() and (prob == 1.0).any()
    assert np.abs(logit).max() > 1e4  # exp overflowed and underflowed
    check_against_host(big, prob, logit, full[2], "coef * 1e6")


def test_invalid_tables_and_states_set_status(gpu, packed, tmp_path):
    states, sets = packed
    i = 9
    bad_sets = sets[[i, i, i]].copy()
    bad_sets["mask"][0, 2] = N.FSET_SLOTS          # a header out of range
    bad_sets["key"][1, 1, 0] = 400                  # a key off the board
    bad_states = states[[i]].copy()
    bad_states["planes"][0, 1] |= bad_states["planes"][0, 0]  # two players on the same cells
    _, _, status = gpu.winprob_eval(states[[i, i, i]], bad_sets, None, MAX_TURNS, MODEL)
    assert status.tolist() == [N.SNAP_ST_TABLE, N.SNAP_ST_TABLE, 0]
    _, _, status = gpu.winprob_eval(bad_states, sets[[i]], None, MAX_TURNS, MODEL)
    assert status.tolist() == [N.SNAP_ST_STATE]

    # predict_many raises on such a board
    from reinforcementlearning_blokus_amd.engine.board import Player
    from tests.helpers import POS, engine_board
    path = tmp_path / "model.json"
    path.write_text(json.dumps(FIX["model"]))
    ev = LearnedWinProbabilityEvaluator(str(path))
    good = engine_board(POS[FIX["positions"][i]["index"]])
    assert ev.predict_many([good]).shape == (1, 4)
    broken = good.copy()
    broken.frontier_tables["mask"][0, 2] = N.FSET_SLOTS
    with pytest.raises(RuntimeError, match="board 1 .*status 1"):
        ev.predict_many([good, broken])
    overlap = good.copy()
    overlap.player_bits[Player.BLUE] |= overlap.player_bits[Player.RED]
    with pytest.raises(RuntimeError, match="board 0 .*status 2"):
        ev.predict_many([overlap, good])
    with pytest.raises(RuntimeError):
        ev.predict_player_win_probability(overlap, Player.RED)


def test_model_checks_on_a_live_handle(gpu, packed, full):
    states, sets = packed
    h, L = gpu.handle, N.load()
    prob, status = np.zeros((1, 4)), np.zeros(1, np.uint8)
    mask = np.zeros(1, np.uint8)
    gpu.handle.has_moves(states[:1].ctypes.data, 1, mask.ctypes.data, N.MEM_HOST)
    last = gpu.last_kernel()
    assert last != "k_winprob"

    def call(model, max_turns=MAX_TURNS, n=1, st=states[:1].ctypes.data):
        return L.bk_winprob_eval(h.ptr, C.c_void_p(st), C.c_void_p(sets[:1].ctypes.data), n, None, max_turns,
                                 C.byref(model), C.c_void_p(prob.ctypes.data), None, C.c_void_p(status.ctypes.data),
                                 N.MEM_HOST)

    good = WinProbModel.from_dict(FIX["model"]).as_native()
    for field, k, value, word in (("coef", 3, math.nan, "non-finite"), ("mean", 0, math.inf, "non-finite"),
                                  ("scale", 33, 0.0, "scale of 0"), ("scale", 5, -math.inf, "non-finite")):
        bad = WinProbModel.from_dict(FIX["model"]).as_native()
        getattr(bad, field)[k] = value
        assert call(bad) == N.EINVAL and word in h.error(), (field, h.error())
    bad = WinProbModel.from_dict(FIX["model"]).as_native()
    bad.intercept = math.nan
    assert call(bad) == N.EINVAL and "intercept" in h.error()
    assert call(good, max_turns=-1) == N.EINVAL and "max_turns" in h.error()
    assert call(good, st=None) == N.EINVAL
    assert call(good, n=0) == N.OK
    # device pointers: the documented alignments (checked before anything is read)
    import torch
    d = torch.zeros(8192, dtype=torch.uint8, device="cuda:0")
    base = (d.data_ptr() + 255) & ~255
    dev = dict(st=base, fs=base + 1024, ti=base + 4096, prob=base + 4352, logit=base + 5120, status=base + 6144)

    def dcall(n=1, **kw):
        a = dict(dev, **kw)
        return L.bk_winprob_eval(h.ptr, C.c_void_p(a["st"]), C.c_void_p(a["fs"]), n, C.c_void_p(a["ti"]), MAX_TURNS,
                                 C.byref(good), C.c_void_p(a["prob"]), C.c_void_p(a["logit"]),
                                 C.c_void_p(a["status"]), N.MEM_DEVICE)

    for name, off in (("fs", 8), ("st", 4), ("prob", 4), ("logit", 4), ("ti", 2)):
        assert dcall(**{name: dev[name] + off}) == N.EINVAL and "aligned" in h.error(), name
    assert dcall(n=0) == N.OK and dcall(n=0, status=dev["status"] + 1) == N.OK  # status is bytes
    assert gpu.last_kernel() == last and not prob.any()  # none of these launched or wrote
    assert call(good) == N.OK and gpu.last_kernel() == "k_winprob"
    assert prob.tobytes() == full[0][:1].tobytes()


def test_evaluator_api(tmp_path, full):
    from reinforcementlearning_blokus_amd.engine.board import Player
    from tests.helpers import POS, engine_board
    path = tmp_path / "model.json"
    path.write_text(json.dumps(FIX["model"]))
    pick = [i for i, r in enumerate(FIX["positions"]) if r["index"] is not None]
    pick = [pick[0], pick[len(pick) // 3], pick[2 * len(pick) // 3], pick[-1]]
    boards = [engine_board(POS[FIX["positions"][i]["index"]]) for i in pick]
    ev = {mode: LearnedWinProbabilityEvaluator(str(path), potential_mode=mode) for mode in ("prob", "logit")}
    many = ev["prob"].predict_many(boards)
    assert many.tobytes() == full[0][pick].tobytes()  # the Board route packs the fixture's states and tables
    assert ev["prob"].predict_many([]).shape == (0, 4)
    for b, i in zip(boards, pick):
        r = FIX["positions"][i]
        bounds = logit_bounds(MODEL, r["rows"])
        for p in Player:
            k = p.value - 1
            got = ev["prob"].predict_player_win_probability(b, p)
            assert type(got) is float and got == float(full[0][i, k])
            tol = max(bounds[k]) / 4 + 4 * EPS
            assert abs(got - r["prob"][k]) <= tol
            assert abs(ev["prob"].potential(b, p) - r["potential_prob"][k]) <= tol
            # log(c / (1 - c)) of the clipped c: slope 1 / (c (1 - c)), then three roundings
            c = min(max(r["prob"][k], 1e-6), 1 - 1e-6)
            tol_logit = 1.01 * tol / (c * (1 - c)) + 4 * EPS * max(1.0, abs(r["potential_logit"][k]))
            assert abs(ev["logit"].potential(b, p) - r["potential_logit"][k]) <= tol_logit
    dummy = LearnedWinProbabilityEvaluator("dummy_model.json")
    assert dummy.predict_player_win_probability(boards[0], Player.RED) == 0.5
    assert dummy.predict_many(boards).tolist() == [[0.5] * 4] * len(boards)
