"""tests/scan_reference.py against the reference's own recordings, and the conditions the
edge-board set (tests/edge_boards.py) has to meet.  No GPU.

Every restated field of bk_player_metrics, bk_snapshot_rec and bk_step_rec is compared on
every record of tests/golden/telemetry.json (`ints`, k = 3 and the k = 8 subset),
winprob_features.json and steplog_steps.json: positions that play produced, recorded from
the reference.  A field that reproduces every record may referee the kernels on boards the
reference never saw (tests/test_gpu_scan_edges_*.py).  Tolerance: exact.
"""
import base64
import random
import zlib

import numpy as np
import pytest

from oracle import pyoracle as O
from reinforcementlearning_blokus_amd import _native as N
from tests import edge_boards as E
from tests import rules_reference as R
from tests import scan_reference as S
from tests.conftest import load_golden
from tests.helpers import POS, oracle_fset, pack_many, replay

TEL = load_golden("telemetry.json")
SNAP = load_golden("winprob_features.json")
STEPS = load_golden("steplog_steps.json")


def _decode(text, dtype):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype=dtype).copy()


def _masks(state):
    return [R.legal_mask_plain(state, q) for q in range(4)]


def test_shuffle_counted_is_cpythons_shuffle():
    a, b = random.Random(42), random.Random(42)
    for n in (1, 2, 3, 58, 678, 2048):
        want = list(range(n))
        a.shuffle(want)
        got, draws = S.shuffle_counted(b, n)
        assert got == want and draws >= n - 1
        assert a.getstate() == b.getstate()


@pytest.fixture(scope="module")
def telemetry_positions():
    """(state, sets, board, masks) of every telemetry fixture position, through the oracle's
    replay of the recorded placements (the reference's table layouts)."""
    out = []
    for rec in TEL["positions"]:
        b = replay(rec if rec["index"] is None else POS[rec["index"]])
        st = pack_many([b])[0]
        out.append((st, oracle_fset(b), b, _masks(st)))
    return out


def test_telemetry_fields_equal_the_recordings(telemetry_positions):
    n = 0
    for rec, (st, fs, b, masks) in zip(TEL["positions"], telemetry_positions):
        for mode, k in (("fast", 3), ("k8", 8)):
            if mode not in rec:
                continue
            assert rec[mode]["k"] == k
            for p in range(4):
                want = rec[mode]["ints"][p]
                got = S.telemetry_record(st, fs, p, masks=masks, k_samples=k, board=b)
                assert got["status"] == 0
                for f in S.TEL_PHASE_A + ("sample_index", "sample_mobility", "rng_draws"):
                    assert got[f] == want[f], (rec["num_moves"], rec["seed"], mode, p, f, got[f], want[f])
                assert got["n_samples"] == len(want["sample_index"])
                n += 1
    assert n >= 4 * len(TEL["positions"]) + 4 * 7


def test_snapshot_fields_equal_the_recordings():
    for rec in SNAP["positions"]:
        st = _decode(rec["state"], N.STATE_DTYPE)[0]
        fs = _decode(rec["sets"], N.FSET_DTYPE)[0]
        masks = _masks(st)
        for p in range(4):
            got = S.snapshot_record(st, fs, p, masks=masks)
            for f in S.SNAP_FIELDS:
                assert got[f] == rec["ints"][p][f], (rec["num_moves"], rec["seed"], p, f, got[f], rec["ints"][p][f])
            assert S.pieces_used(st, p) == sorted(rec["used"][p])


def test_steplog_fields_equal_the_recordings():
    assert sorted(S.STEP_FIELDS) == sorted(STEPS["rec_fields"])
    for c in STEPS["cases"]:
        before = _decode(c["before"]["state"], N.STATE_DTYPE)[0]
        after = _decode(c["after"]["state"], N.STATE_DTYPE)[0]
        sb = _decode(c["before"]["sets"], N.FSET_DTYPE)[0]
        sa = _decode(c["after"]["sets"], N.FSET_DTYPE)[0]
        step = np.zeros(1, dtype=N.STEP_DTYPE)[0]
        step["mover"], step["piece_id"], step["orientation"], step["anchor_row"], step["anchor_col"] = c["step"]
        got = S.step_record(before, sb, after, sa, step)
        for f in S.STEP_FIELDS:
            assert got[f] == c["ints"][f], (c["num_moves"], c["seed"], c["step"], f, got[f], c["ints"][f])


def test_step_of_move_round_trips():
    for g in range(N.N_ORIENTS):
        step = S.step_of_move(2, g * 400 + 7 * 20 + 3)
        assert S.step_cells(step) == S.move_cells(g * 400 + 7 * 20 + 3)
        assert (int(step["mover"]), int(step["anchor_row"]), int(step["anchor_col"])) == (2, 7, 3)


# ------------------------------------------------------------------------------ the board set


def test_edge_board_set_meets_its_conditions():
    st, fs, masks, cnt = E.edge_states(), E.edge_sets(), E.edge_masks(), E.edge_counts()
    assert len(st) == len(fs) == 43 and cnt.shape == (43, 4)
    # every orientation has a legal anchor with its box on each edge, on the random-bit part
    hits = R.edge_pairs_hit(st[:E.N_RANDOM], masks[:E.N_RANDOM])
    assert hits.shape == (91, 4) and (hits > 0).all(), np.argwhere(hits == 0).tolist()
    # lists past the 2,048 cap, none exactly at it
    over = int((cnt[:E.N_SEARCH] > E.CAP).sum())
    print("board-players", cnt.size, "moves", int(cnt.min()), "...", int(cnt.max()), "above the cap", over)
    assert over >= 20 and not (cnt == E.CAP).any() and cnt.max() > 2800
    assert (cnt == 0).any() and (cnt == 1).any()
    # every table fits the record (oracle_fset asserts it slot for slot) and holds the plain
    # rule's moves: the oracle's frontier-order list is the same set
    assert (fs["mask"] < N.FSET_SLOTS).all()
    boards = E.edge_boards()

    def same(k):
        i, p = divmod(k, 4)
        return sorted(O.legal_moves(boards[i], p, O.ORDER_FRONTIER)) == np.flatnonzero(masks[i, p]).tolist()

    assert all(E.pool_map(same, range(4 * len(st))))
    # the telemetry run: both kinds of record in number, no clean one near the MT table's end
    status = [S.telemetry_status(cnt[i].tolist(), p) for i in range(len(st)) for p in range(4)]
    flagged = sum(1 for s, _ in status if s == N.TEL_ST_LIST)
    clean = [d for s, d in status if s == 0]
    print("telemetry records flagged", flagged, "clean", len(clean), "most draws of a clean one", max(clean))
    assert flagged >= 32 and len(clean) >= 32 and flagged + len(clean) == len(status)
    assert max(clean) < N.TEL_MT_OUTPUTS
