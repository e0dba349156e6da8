"""k_rollout_fr's live-slot masks carried from ply to ply (csrc/blokus_kernels.hip:
live_masks, copy_fset_in_live / init_live_masks, FsMix::put, fs_resize_mix,
locate_move_frontier<2, true>).

The playout kernel keeps, per player, a 128-bit mask of the slots of the CPython frontier
table that hold a key (tables of <= 128 slots): in spare words of the slab with Philox
draws, in the record's padding when the compat RNG owns those words.  It is built once
when a game starts, every set operation flips its slot's bit, a resize replaces it by the
new table's occupancy, and locate walks the table by it instead of reading every slot.  A
wrong bit makes locate skip a frontier cell or read a dead slot, which changes the anchor
drawn and so the state after the ply and every later table.  States, tables and records
are compared here, exactly.

The cases follow tests/test_gpu_place_onepass.py, whose builders they share: 64 roots,
one per lane of a wave, 64 playouts per launch; tables that random play does not reach
are rebuilt through bk_debug_fset_op (never by writing slots).  Each case runs
* a SEM_ADVANCE launch of PLIES = 12 placements, so every player moves again (three
  times) on a mask carried from its last move: states and all four tables, slot for slot,
  against the oracle's replay of the same Philox streams;
* a SEM_ARENA launch to the end of the game: records byte for byte, final states and
  tables.
test_case_contains_its_situation asserts, from the oracle alone, that the fixture holds
what the case is named after.  Tolerance: exact.

Not built (issue case 4, first three items): a lone live key in slot 0, a lone live key
in slot 127, and all live keys in slots 96..127 of a 128-slot table.  A mover's table must
hold the mover's true frontier cells (the kernel derives membership from the board): a
player with one frontier cell is a player at its first move, whose key is its start
corner, and the slots of a mid-game mover's dozen or more cells follow from CPython's
tuple hash, so neither the number of live keys nor their slots can be chosen by the
builders without breaking that premise.  The reachable neighbours are tested instead: the first move
of a game (a single live key, the start corner, in an 8-slot table: cases carry and
resizes), and in 128-slot tables a live key in slot 0, a live key in slot 127, and a key
added and a key discarded in each of the four 32-bit words (case words).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle as O
from reinforcementlearning_blokus_amd import _native as N
from tests.helpers import oracle_fset, oracle_states, pack_many
from tests.test_gpu_place_onepass import (Case, _assert_tables, _can_move, _join, _members_with_stale, _mover_mask,
                                          _oracle_roots, _pack, _reshape_mover, _reshape_until)

SEED = 9900
PLIES = 12  # placements per SEM_ADVANCE launch: each player moves three times


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


def _keys(b, p):
    return np.array(b.fr[p].key[: b.fr[p].mask + 1], dtype=np.int16)


def _ply_tables(c, pid):
    """Playout pid's placements over the case's plies: [(mover, slots before, slots after)]."""
    g = int(c.idx[pid])
    b = O.board_from(c.st[g].tobytes(), c.fs[g])
    _, tr = O.playout_arena_philox(b, c.seed, pid, O.ORDER_FRONTIER, max_plies=c.plies)
    w = O.board_from(c.st[g].tobytes(), c.fs[g])
    cur, out = w.cur, []
    for mv in tr:
        if mv >= 0:
            k0 = _keys(w, cur)
            O.place_move(w, cur, mv)
            out.append((cur, k0, _keys(w, cur)))
        cur = (cur + 1) & 3
    return out


def _resizes(c, pid):
    """(mask before, mask after) of the placements of playout pid that rebuilt the table
    (a resize re-inserts in slot order: the slots move, or the dummies go)"""
    return [(len(k0) - 1, len(k1) - 1) for _, k0, k1 in _ply_tables(c, pid)
            if len(k0) != len(k1) or ((k0 == -2).sum() > 0 and (k1 == -2).sum() == 0)]


def _moves_again(c, pid):
    """placements in playout pid by a player that has already moved in the launch"""
    seen, n = set(), 0
    for p, _, _ in _ply_tables(c, pid):
        n += p in seen
        seen.add(p)
    return n


def _take(st, fs, want, have=()):
    return [g for g in range(len(st)) if g not in have and want(g)]


def _build_carry():
    st0, fs0 = _oracle_roots(2, 64)    # the mover has not moved yet: 8 slots, one key
    st, fs = _oracle_roots(24, 256)
    by = {m: _take(st, fs, lambda g, m=m: _mover_mask(st, fs, g) == m)[:16] for m in (31, 63, 127)}
    for g in _take(st, fs, lambda g: _mover_mask(st, fs, g) == 31)[16:32]:  # (128-slot tables are rare at 24 plies)
        if len(by[127]) < 16:
            _reshape_mover(st, fs, g, 128)
            by[127].append(g)
    rest = 64 - 16 - len(by[31]) - len(by[63]) - len(by[127])
    st, fs = _join([(st0, fs0, range(16 + rest)), (st, fs, by[31] + by[63] + by[127])])
    return Case("carry", st, fs, 64, PLIES, SEED + 1)


def _build_resizes():
    st0, fs0 = _oracle_roots(2, 64)     # 8 -> 32 at the mover's first move
    st, fs = _oracle_roots(24, 256)
    st2, fs2 = _oracle_roots(40, 256)
    small = _take(st, fs, lambda g: _mover_mask(st, fs, g) <= 63 and len(_members_with_stale(st, fs, g, 0)) <= 15)
    up = small[:10]       # 32 -> 128: 32 slots, 17 live keys, fill at the threshold
    keep = small[10:20]   # dummy-heavy: 64 slots, fill at the threshold, < 16 live keys
    mid = _take(st2, fs2, lambda g: _mover_mask(st2, fs2, g) == 63 and _can_move(st2, fs2, g)
                and len(_members_with_stale(st2, fs2, g, 22)) >= 20)[:10]  # 64 -> 128: the stage overflows
    for lane, g in enumerate(up, 16):
        _reshape_until(st, fs, g, 32, 18, 17, SEED + 2, lane, 127)
    for lane, g in enumerate(keep, 26):
        n = len(_members_with_stale(st, fs, g, 0))
        _reshape_until(st, fs, g, 64, 37, n, SEED + 2, lane, 31 if n < 7 else 63)
    for lane, g in enumerate(mid, 36):
        _reshape_until(st2, fs2, g, 64, 37, 22, SEED + 2, lane, 127)
    other = _take(st, fs, lambda g: True, have=up + keep)[: 64 - 46]
    st, fs = _join([(st0, fs0, range(16)), (st, fs, up + keep), (st2, fs2, mid), (st, fs, other)])
    return Case("resizes", st, fs, 64, PLIES, SEED + 2)


def _build_grow_return():
    st, fs = _oracle_roots(24, 256)
    st2, fs2 = _oracle_roots(48, 256)
    ok = _take(st2, fs2, lambda g: _can_move(st2, fs2, g))
    grow = [g for g in ok if len(_members_with_stale(st2, fs2, g, 44)) >= 38][:8]   # 128 -> 256
    back = [g for g in ok if g not in grow and len(_members_with_stale(st2, fs2, g, 0)) <= 24][:8]  # 256 -> <= 128
    for lane, g in enumerate(grow, 20):
        _reshape_until(st2, fs2, g, 128, 76, 44, SEED + 3, lane, 255)
    for lane, g in enumerate(back, 28):
        n = max(20, len(_members_with_stale(st2, fs2, g, 0)))
        _reshape_until(st2, fs2, g, 256, 152, n, SEED + 3, lane, 127)
    rest = list(range(48))
    st, fs = _join([(st, fs, rest[:20]), (st2, fs2, grow + back), (st, fs, rest[20:])])
    return Case("grow_return", st, fs, 64, PLIES, SEED + 3)


def _build_words():
    st, fs = _oracle_roots(24, 64)
    for g in range(64):
        if _mover_mask(st, fs, g) != 127:
            _reshape_mover(st, fs, g, 128)
    return Case("words", st, fs, 64, PLIES, SEED + 4)


def _build_idle():
    st, fs = _oracle_roots(56, 256)
    idle = _take(st, fs, lambda g: not _can_move(st, fs, g))[:16]
    late = _take(st, fs, lambda g: True, have=idle)[:24]  # these games end within the plies
    st2, fs2 = _oracle_roots(40, 256)                     # and these go on
    st, fs = _join([(st, fs, sorted(idle + late)[:20]), (st2, fs2, range(24)), (st, fs, sorted(idle + late)[20:])])
    return Case("idle", st, fs, 64, PLIES, SEED + 5)


_BUILDERS = {"carry": _build_carry, "resizes": _build_resizes, "grow_return": _build_grow_return,
             "words": _build_words, "idle": _build_idle}
_CASES = {}


@pytest.fixture(scope="module", params=list(_BUILDERS))
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = _BUILDERS[request.param]()
    return request.param, _CASES[request.param]


# ---------------------------------------------------------------- the inputs (oracle only)
def test_case_contains_its_situation(case):
    """From the oracle's replay alone: the table sizes, the resizes within the tested plies
    and the key positions the case is named after, and movers that move again on a carried
    mask."""
    name, c = case
    first, passes = c.first_moves()
    rs = [r for pid in range(64) for r in _resizes(c, pid)]
    again = [_moves_again(c, pid) for pid in range(64)]
    if name != "idle":  # (idle: late games, see below)
        assert sum(a >= 8 for a in again) >= 56, again  # 12 placements: 8 of them on a carried mask
    if name == "carry":
        assert {8, 32, 64, 128} <= {f[0] + 1 for f in first}, first
        roots_dummies = sum(int(c.fs[g]["fill"][int(c.st[g]["current_player"])]) >
                            int(c.fs[g]["used"][int(c.st[g]["current_player"])]) for g in range(64))
        assert roots_dummies >= 16, roots_dummies
        assert sum(f[0] == 7 for f in first) >= 8 and sum(f[0] == 127 for f in first) >= 8, first
    elif name == "resizes":
        assert sum(r == (7, 31) for r in rs) >= 8, rs  # (a first move leaves the 8 slots: the second resizes)
        assert sum(f[:2] == (31, 127) for f in first) >= 2, first
        assert sum(f[:2] == (63, 127) for f in first) >= 2, first     # the stage overflows: a restart
        kept = [pid for pid in range(26, 36) if _resizes(c, pid)[:1] in ([(63, 63)], [(63, 31)])]
        assert len(kept) >= 2, [_resizes(c, pid)[:1] for pid in range(26, 36)]
        assert len(rs) >= 100, len(rs)
    elif name == "grow_return":
        assert sum(f[:2] == (127, 255) for f in first) >= 2, first    # the mask is dropped
        assert sum(f[0] == 255 and f[1] <= 127 for f in first) >= 2, first  # and made again by the resize
        # a 256-slot table is walked the old way when its player moves again
        assert sum(any(len(k0) == 256 for _, k0, _ in _ply_tables(c, pid)[1:]) for pid in range(64)) >= 2
    elif name == "words":
        assert all(f[0] == 127 for f in first), first
        added, gone, slot0, slot127 = set(), set(), 0, 0
        for pid in range(64):
            moved = set()
            for p, k0, k1 in _ply_tables(c, pid):
                if len(k0) == len(k1) == 128:
                    added |= {int(s) >> 5 for s in np.flatnonzero((k0 < 0) & (k1 >= 0))}
                    gone |= {int(s) >> 5 for s in np.flatnonzero((k0 >= 0) & (k1 < 0))}
                    if p in moved:  # this ply's locate walks a mask carried from p's last move
                        slot0 += int(k0[0] >= 0)
                        slot127 += int(k0[127] >= 0)
                moved.add(p)
        assert added == gone == {0, 1, 2, 3}, (added, gone)
        assert slot0 >= 1 and slot127 >= 1, (slot0, slot127)
    elif name == "idle":
        assert passes >= 8, passes
        placed = [sum(e is not None for e in ev) for _, ev, _, _ in c.ref]
        assert sum(n < PLIES for n in placed) >= 8 and sum(n == PLIES for n in placed) >= 8, placed  # finished / busy
        assert sum(any(e is None for e in ev) and _moves_again(c, pid) >= 1
                   for pid, (_, ev, _, _) in enumerate(c.ref)) >= 8  # a pass, then a move on the mask it left alone


# ---------------------------------------------------------------- the GPU against the oracle
@pytest.mark.gpu
def test_tables_after_the_plies_match_oracle(gpu, case):
    """One SEM_ADVANCE launch of PLIES placements: states and all four tables."""
    name, c = case
    out_st, out_fs, res = gpu.rollout_frontier(c.st, c.fs, len(c.idx), semantics=N.SEM_ADVANCE, rng=N.RNG_PHILOX,
                                               seed=c.seed, max_plies=c.plies, root_index=c.idx, with_results=True)
    assert gpu.last_kernel() == "k_rollout_fr"
    want = _pack([b for b, _, _, _ in c.ref])
    for pid in range(len(c.idx)):
        assert int(res[pid]["status"]) & 2 == 0, pid
        for f in ("planes", "used", "first_move", "current_player", "move_count"):
            assert np.array_equal(out_st[pid][f], want[pid][f]), (pid, f)
        _assert_tables(out_fs[pid], c.ref[pid][0], pid)


@pytest.mark.gpu
def test_full_playouts_match_oracle(gpu, case):
    """One SEM_ARENA launch from the same roots to the end of the games: records byte for
    byte, final states and final tables."""
    name, c = case
    out_st, out_fs, res = gpu.rollout_frontier(c.st, c.fs, len(c.idx), semantics=N.SEM_ARENA, rng=N.RNG_PHILOX,
                                               seed=c.seed, root_index=c.idx, with_states=True)
    want = _pack([e for _, _, e, _ in c.ref])
    for pid in range(len(c.idx)):
        assert res[pid].tobytes() == c.ref[pid][3], pid
        for f in ("planes", "used", "first_move", "move_count"):
            assert np.array_equal(out_st[pid][f], want[pid][f]), (pid, f)
        _assert_tables(out_fs[pid], c.ref[pid][2], pid)


# ---------------------------------------------------------------- slot reuse
@pytest.mark.gpu
def test_second_game_on_a_used_record():
    """One resident block per CU and nslots + 65 playouts: 65 slots start a second game on
    a record (slab and tables) that holds the first game's masks.  About 100 records from
    both rounds, the round boundary included, against the oracle."""
    import torch
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    with pytest.MonkeyPatch.context() as monkeypatch:
        monkeypatch.setenv("BK_BLOCKS_PER_CU", "1")
        monkeypatch.setenv("BK_FR_BLOCKS_PER_CU", "1")
        monkeypatch.delenv("BK_HANDOUT", raising=False)
        gpu = BlokusGPU(0)  # the library reads the environment once, when the handle is created
    nslots = torch.cuda.get_device_properties(0).multi_processor_count * 256
    boards = oracle_states(64, seed0=9100, lo=40, hi=40)
    st, fs = pack_many(boards), np.array([oracle_fset(b) for b in boards], dtype=N.FSET_DTYPE)
    n = nslots + 65
    idx = (np.arange(n) % 64).astype(np.int32)
    res = gpu.rollout_frontier(st, fs, n, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED, root_index=idx)
    assert gpu.last_kernel() == "k_rollout_fr"
    gpu.synchronize()
    ids = set(np.linspace(0, n - 1, 64).astype(np.int64).tolist()) | set(range(nslots - 8, n, 2)) | {nslots - 1, nslots}

    def one(pid):
        b = O.board_from(st[int(idx[pid])].tobytes(), fs[int(idx[pid])])
        r, _ = O.playout_arena_philox(b, SEED, pid, O.ORDER_FRONTIER)
        return pid, bytes(r)

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(one, sorted(ids)))
    bad = [pid for pid, rb in refs if res[pid].tobytes() != rb]
    assert 96 <= len(refs) <= 110 and not bad, (len(refs), len(bad), bad[:8])


def test_second_game_sample_covers_both_rounds():
    """(oracle-free condition on the sample above: ids on both sides of a round boundary
    for any grid size)"""
    for nslots in (256 * 64, 256 * 256, 256 * 304):
        n = nslots + 65
        ids = set(np.linspace(0, n - 1, 64).astype(np.int64).tolist()) | set(range(nslots - 8, n, 2)) | {nslots - 1, nslots}
        assert sum(i >= nslots for i in ids) >= 30 and sum(i < nslots for i in ids) >= 60 and max(ids) == n - 1


# ---------------------------------------------------------------- masks of re-laid tables
def _rollout_a_roots():
    """The carry case's roots: tables of 8 to 128 slots, many with dummies, which
    Board.copy() lays out anew at the start of an MCTS rollout."""
    if "carry" not in _CASES:
        _CASES["carry"] = _build_carry()
    return _CASES["carry"]


def test_rollout_a_roots_are_relaid_by_the_copy():
    """(oracle only) the copy changes the layout of most of these tables: another size, or
    the dummies gone, so the masks cannot be the root's"""
    c = _rollout_a_roots()
    relaid = 0
    for g in range(64):
        for p in range(4):
            m, f, u = (int(c.fs[g][k][p]) for k in ("mask", "fill", "used"))
            size = 8
            if u * 5 >= 21:
                while size <= 2 * u:
                    size <<= 1
            relaid += size - 1 != m or f != u
    assert relaid >= 64, relaid


@pytest.mark.gpu
def test_mcts_rollouts_build_masks_after_the_copy(gpu):
    """SEM_ROLLOUT (MCTSAgent._rollout on board.copy()): the tables are laid out anew by
    fs_copy_dev and their masks come from init_live_masks.  64 rollouts of up to 50 moves
    against the oracle's rollouts: rewards and plies."""
    c = _rollout_a_roots()
    seeds = np.array([[(pid * 40503 + SEED) % 2**31] * 4 for pid in range(64)], dtype=np.uint32)
    res = gpu.rollout_frontier(c.st, c.fs, 64, semantics=N.SEM_ROLLOUT, rng=N.RNG_NUMPY_MT, compat_seeds=seeds,
                               root_index=c.idx, max_plies=50, seats_share_stream=True)
    assert gpu.last_kernel() == "k_rollout_fr"
    assert (res["status"] == 0).all()

    def one(pid):
        b = O.board_from(c.st[pid].tobytes(), c.fs[pid])
        return O.rollout_a(b, b.cur, int(seeds[pid][0]), O.ORDER_FRONTIER, 50)

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(one, range(64)))
    got = [(int(r["reward"]), int(r["plies"])) for r in res]
    bad = [pid for pid in range(64) if got[pid] != refs[pid]]
    assert not bad, (bad[:8], got[bad[0]], refs[bad[0]])
    assert sum(pl >= 8 for _, pl in refs) >= 48  # long enough for every player to move again


# ---------------------------------------------------------------- the mode without stored masks
@pytest.mark.gpu
def test_compat_rng_launch_keeps_masks_in_the_padding(gpu):
    """BK_RNG_NUMPY_MT: the slab words of the masks hold the seats' MT cursors, so
    k_rollout_fr keeps the masks in the record's padding instead.  64 playouts of the
    carry case's roots against the oracle's compat playouts: scores, winners, passes and
    turns (what tests/test_gpu_frontier.py compares of compat playouts)."""
    if "carry" not in _CASES:
        _CASES["carry"] = _build_carry()
    c = _CASES["carry"]
    seeds = ((np.arange(64 * 4, dtype=np.uint64).reshape(64, 4) * 40503 + SEED) % 2**31).astype(np.uint32)
    res = gpu.rollout_frontier(c.st, c.fs, 64, semantics=N.SEM_ARENA, rng=N.RNG_NUMPY_MT, compat_seeds=seeds,
                               root_index=c.idx)
    assert gpu.last_kernel() == "k_rollout_fr"
    assert (res["status"] == 0).all()

    def one(pid):
        b = O.board_from(c.st[pid].tobytes(), c.fs[pid])
        r, _ = O.playout_arena(b, [int(s) for s in seeds[pid]], O.ORDER_FRONTIER)
        return list(r.scores), r.winner_mask, r.passes, r.turns

    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(one, range(64)))
    got = [(list(r["scores"]), int(r["winner_mask"]), int(r["passes"]), int(r["turns"])) for r in res]
    bad = [pid for pid in range(64) if got[pid] != refs[pid]]
    assert not bad, (bad[:8], got[bad[0]], refs[bad[0]])
