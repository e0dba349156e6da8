"""bk_advance and the frontier-order ADVANCE deep into the game, and bk_state.out_mask.

Past 20 plies the ADVANCE paths of rollout_body (csrc/blokus_kernels.hip) do things the
20-ply root tests never reach: players pass, the run stops early once nobody can move,
the player left to move at the end of the budget may be stuck, store_state writes a
non-zero out_mask ("bit p: p is known to have no legal move"), start_game reads it back
for ARENA / ADVANCE runs, and the frontier tables resize to 128 slots.  The referee is
the oracle's Philox replay of the same streams (generate_random_valid_state's loop,
tests/utils_game_states.py:12-57, and the arena loop, arena_runner.py:652-697); the
out_mask hint is also checked for what it promises on its own.  Tolerance: exact.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle as O
from reinforcementlearning_blokus_amd import _native as N
from tests import rules_reference as R

pytestmark = pytest.mark.gpu

SEED = 4242
GAMES = 64
PLIES = (48, 56, 64, 84)
FIELDS = ("planes", "used", "first_move", "current_player", "move_count")


@pytest.fixture(scope="module")
def gpu():
    from reinforcementlearning_blokus_amd.gpu import BlokusGPU
    return BlokusGPU(0)


def _pool_map(fn, items):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(fn, items))


@pytest.fixture(scope="module")
def oracle_late():
    """plies -> the oracle's 64 boards after bk_advance's budget of `plies` placements on
    Philox streams (SEED, 0..63), with each player's number of legal moves."""
    def one(arg):
        plies, pid = arg
        b = O.new_board()
        O.playout_arena_philox(b, SEED, pid, O.ORDER_NAIVE, max_plies=plies)
        return b, [len(O.legal_moves(b, p, O.ORDER_NAIVE)) for p in range(4)]

    out = _pool_map(one, [(plies, pid) for plies in PLIES for pid in range(GAMES)])
    return {plies: out[k * GAMES:(k + 1) * GAMES] for k, plies in enumerate(PLIES)}


@pytest.fixture(scope="module")
def gpu_late(gpu):
    from reinforcementlearning_blokus_amd.gpu import empty_state
    return {plies: gpu.advance(empty_state(), GAMES, plies, seed=SEED, root_index=np.zeros(GAMES, np.int32))
            for plies in PLIES}


def test_oracle_set_holds_passes_early_stops_and_stuck_movers(oracle_late):
    """The condition on the inputs, on the oracle side: the set contains games that
    stopped before their budget (nobody could move) and games that used the whole budget
    and end on a player who cannot move; at 84 plies every game stops early."""
    early = stuck = 0
    for plies in PLIES:
        for b, cnt in oracle_late[plies]:
            if b.move_count < plies:
                early += 1
                assert sum(cnt) == 0
            elif cnt[b.cur] == 0 and sum(cnt) > 0:
                stuck += 1
    print("early stops", early, "budget ends on a stuck player", stuck)
    assert early > 0 and stuck > 0
    assert all(b.move_count == 48 for b, _ in oracle_late[48])
    assert all(b.move_count < 84 for b, _ in oracle_late[84])


@pytest.mark.parametrize("plies", PLIES)
def test_advance_equals_oracle_replay(gpu_late, oracle_late, plies):
    """bk_advance(empty board, 64 games, plies) against the oracle's replay, field for
    field: the pass handling, the early stop and the player left to move.  (With the
    budget used the seat after the last mover is left to move even if it is known to be
    stuck: generate_random_valid_state leaves its loop before looking at that player.
    rollout_body once let known-stuck seats pass first, which only shows past ~40 plies.)"""
    st = gpu_late[plies]
    ref = np.frombuffer(bytes(O.states_array([b for b, _ in oracle_late[plies]])), dtype=N.STATE_DTYPE)
    for f in FIELDS:
        bad = np.flatnonzero((st[f] != ref[f]).reshape(GAMES, -1).any(axis=1))
        assert not len(bad), (f, bad[:8].tolist(), st[f][bad[:4]].tolist(), ref[f][bad[:4]].tolist())


@pytest.mark.parametrize("plies", PLIES)
def test_advance_out_mask_and_state_sanity(gpu_late, oracle_late, plies):
    """What out_mask promises (include/blokus_hip.h): a set bit means that player has no
    legal move -- the oracle finds none on its own board and the plain rule finds none on
    the returned state; a game that stopped below its budget has all four bits.  And the
    returned state is a position: disjoint planes, move_count = used pieces, each
    player's cells = the sizes of its used pieces, first_move bit p iff p placed nothing."""
    st = gpu_late[plies]
    sizes = R.piece_sizes()
    for i in range(GAMES):
        s = st[i]
        om = int(s["out_mask"])
        assert om <= 0xF and int(s["flags"]) == 0
        _, cnt = oracle_late[plies][i]
        for p in range(4):
            if om >> p & 1:
                assert cnt[p] == 0, (i, p, om)
                assert not R.legal_mask_plain(s, p).any(), (i, p, om)
        if int(s["move_count"]) < plies:
            assert om == 0xF, (i, om)
        grids = R.state_grids(s)
        assert grids.sum(axis=0).max() <= 1
        used = [int(u) for u in s["used"]]
        assert all(u >> 21 == 0 for u in used)
        assert int(s["move_count"]) == sum(bin(u).count("1") for u in used)
        for p in range(4):
            assert int(grids[p].sum()) == sum(sizes[k + 1] for k in range(21) if used[p] >> k & 1), (i, p)
            assert (int(s["first_move"]) >> p & 1) == int(used[p] == 0), (i, p)
    if plies >= 64:
        assert (st["out_mask"] == 0xF).any()


# ---------------------------------------------------------------- the hint changes nothing
@pytest.fixture(scope="module")
def late_roots(gpu_late):
    """The 56- and 64-ply states as roots, as returned and with the hint cleared."""
    hinted = np.concatenate([gpu_late[56], gpu_late[64]])
    assert hinted["out_mask"].any()  # there is a hint to ignore
    plain = hinted.copy()
    plain["out_mask"] = 0
    return hinted, plain


def _ostates(states):
    return (O.State * len(states)).from_buffer_copy(states.tobytes())


def test_arena_playouts_do_not_depend_on_the_hint(gpu, late_roots):
    """Arena playouts (Philox) from the late states: byte-identical records with out_mask
    as returned and zeroed, and (strided) byte-identical to the oracle's playout from the
    unpacked state, which never saw a hint."""
    hinted, plain = late_roots
    n = 4 * len(hinted)
    idx = (np.arange(n) % len(hinted)).astype(np.int32)
    a = gpu.rollout(hinted, n, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED + 1, root_index=idx)
    b = gpu.rollout(plain, n, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED + 1, root_index=idx)
    assert (a["status"] == 0).all()
    assert a.tobytes() == b.tobytes(), np.flatnonzero((a.view(np.uint8).reshape(n, 32) !=
                                                       b.view(np.uint8).reshape(n, 32)).any(axis=1))[:8].tolist()
    assert (a["plies"] == 0).any() and (a["plies"] > 0).any() and (a["passes"] > 0).any()
    ost = _ostates(plain)

    def one(pid):
        r, _ = O.playout_arena_philox(O.unpack(ost[int(idx[pid])]), SEED + 1, pid, O.ORDER_NAIVE)
        return pid, bytes(r)

    bad = [pid for pid, rb in _pool_map(one, list(range(0, n, 3)) + [n - 1]) if a[pid].tobytes() != rb]
    assert not bad, (len(bad), bad[:8])


def test_mcts_rollouts_ignore_the_hint(gpu, late_roots):
    """BK_SEM_ROLLOUT (MCTSAgent._rollout, compat seeds) from the late states: start_game
    ignores out_mask there; rewards and plies equal the oracle's rollout_a, with and
    without the hint, including root players who are already stuck (reward 0, plies 0)."""
    hinted, plain = late_roots
    n = len(hinted)
    idx = np.arange(n, dtype=np.int32)
    seeds = np.repeat((np.arange(n, dtype=np.uint32) * 7919 + 11)[:, None], 4, axis=1)
    runs = [gpu.rollout(roots, n, semantics=N.SEM_ROLLOUT, rng=N.RNG_NUMPY_MT, compat_seeds=seeds, root_index=idx,
                        max_plies=50, seats_share_stream=True) for roots in (hinted, plain)]
    assert runs[0].tobytes() == runs[1].tobytes()
    ost = _ostates(plain)
    refs = _pool_map(lambda i: O.rollout_a(O.unpack(ost[i]), int(plain[i]["current_player"]), int(seeds[i, 0]),
                                           O.ORDER_NAIVE, 50), range(n))
    assert [(int(r["reward"]), int(r["plies"])) for r in runs[0]] == refs
    stuck = [i for i in range(n) if refs[i] == (0, 0)]
    assert stuck and len(stuck) < n  # both kinds of root are in the set (oracle side)
    assert any(int(hinted[i]["out_mask"]) >> int(hinted[i]["current_player"]) & 1 for i in stuck)


@pytest.mark.parametrize("cap", [1, 2, 3, 5])
def test_turn_cap_with_and_without_the_hint(gpu, late_roots, cap):
    """Arena playouts cut by a binding turn cap (max_plies = 1, 2, 3, 5 turns).

    finish_game documents that `passes` / `turns` of a capped record depend on what the
    kernel knew: once all four players are KNOWN stuck the game is over and the record
    carries the reference's discounted counts (passes after the last move dropped, status
    0); stopped by the cap before that, it carries raw counts and status bit 3, and the
    host decides with has_moves.  The hint moves a game from the second kind to the first
    (a root whose out_mask is 0xF is over at once; without the hint the kernel needs four
    turns to find out and the cap comes first), so `passes`, `turns` and `status` may
    differ between the two runs by design.  What the hint may never change is the game
    itself: the moves placed in those turns and the numbers drawn for them, hence
    scores, winner_mask, plies and draws, which must also equal the oracle's capped
    playout.  A record with status bit 3 was stopped by the cap: turns == cap."""
    hinted, plain = late_roots
    n = len(hinted)
    idx = np.arange(n, dtype=np.int32)
    a = gpu.rollout(hinted, n, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED + 2, root_index=idx, max_plies=cap)
    b = gpu.rollout(plain, n, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED + 2, root_index=idx, max_plies=cap)
    for f in ("scores", "winner_mask", "plies", "draws"):
        assert np.array_equal(a[f], b[f]), f
    ost = _ostates(plain)
    refs = _pool_map(lambda i: O.playout_arena_philox(O.unpack(ost[i]), SEED + 2, i, O.ORDER_NAIVE, max_turns=cap)[0],
                     range(n))
    for res in (a, b):
        assert ((res["status"] & ~np.uint8(8)) == 0).all()
        capped = (res["status"] & 8) != 0
        assert (res["turns"][capped] == cap).all()
        assert (res["turns"] <= cap).all() and (res["plies"] <= cap).all()
        for i, r in enumerate(refs):
            assert list(res[i]["scores"]) == list(r.scores) and int(res[i]["winner_mask"]) == r.winner_mask, i
            assert int(res[i]["plies"]) == r.plies and int(res[i]["draws"]) == r.draws, i
    assert ((b["status"] & 8) != 0).any()  # the cap did bind


# ---------------------------------------------------------------- frontier order
FR_PLIES = (48, 60)


@pytest.fixture(scope="module")
def oracle_frontier():
    def one(arg):
        plies, pid = arg
        b = O.new_board()
        O.playout_arena_philox(b, SEED, pid, O.ORDER_FRONTIER, max_plies=plies)
        return b

    out = _pool_map(one, [(plies, pid) for plies in FR_PLIES for pid in range(GAMES)])
    return {plies: out[k * GAMES:(k + 1) * GAMES] for k, plies in enumerate(FR_PLIES)}


@pytest.fixture(scope="module")
def gpu_frontier(gpu):
    from reinforcementlearning_blokus_amd.gpu import empty_state
    return {plies: gpu.rollout_frontier(empty_state(), N.fset_new(1), GAMES, semantics=N.SEM_ADVANCE,
                                        rng=N.RNG_PHILOX, seed=SEED, max_plies=plies,
                                        root_index=np.zeros(GAMES, np.int32))
            for plies in FR_PLIES}


@pytest.mark.parametrize("plies", FR_PLIES)
def test_frontier_advance_states_and_tables_equal_oracle(gpu_frontier, oracle_frontier, plies):
    """k_rollout_fr ADVANCE to 48 / 60 plies: the states field for field and every game's
    four CPython set tables slot for slot (mask, fill, used, key[: mask + 1]).  Condition
    on the oracle side: some table has grown to 128 slots or more, which the 6- and 20-ply
    tests never reach."""
    from tests.helpers import oracle_fset
    st, fs = gpu_frontier[plies]
    boards = oracle_frontier[plies]
    ref = np.frombuffer(bytes(O.states_array(boards)), dtype=N.STATE_DTYPE)
    for f in FIELDS:
        bad = np.flatnonzero((st[f] != ref[f]).reshape(GAMES, -1).any(axis=1))
        assert not len(bad), (f, bad[:8].tolist())
    biggest = 0
    for g in range(GAMES):
        ofs = oracle_fset(boards[g])
        for p in range(4):
            m = int(ofs["mask"][p])
            biggest = max(biggest, m + 1)
            for f in ("mask", "fill", "used"):
                assert int(fs[g][f][p]) == int(ofs[f][p]), (g, p, f)
            assert np.array_equal(fs[g]["key"][p, : m + 1], ofs["key"][p, : m + 1]), (g, p)
    print("largest table", biggest)
    assert biggest >= 128


def test_frontier_arena_playouts_from_late_tables(gpu, gpu_frontier):
    """Frontier-order arena playouts (Philox) from the 48- and 60-ply states and tables:
    strided, byte-identical to the oracle's playout from O.board_from(state, tables)."""
    st = np.concatenate([gpu_frontier[p][0] for p in FR_PLIES])
    fs = np.concatenate([gpu_frontier[p][1] for p in FR_PLIES])
    n = 4 * len(st)
    idx = (np.arange(n) % len(st)).astype(np.int32)
    res = gpu.rollout_frontier(st, fs, n, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED + 3, root_index=idx)
    assert (res["status"] == 0).all()

    def one(pid):
        b = O.board_from(st[int(idx[pid])].tobytes(), fs[int(idx[pid])])
        r, _ = O.playout_arena_philox(b, SEED + 3, pid, O.ORDER_FRONTIER)
        return pid, bytes(r)

    bad = [pid for pid, rb in _pool_map(one, list(range(0, n, 3)) + [n - 1]) if res[pid].tobytes() != rb]
    assert not bad, (len(bad), bad[:8])
    # the hint changes nothing here either
    plain = st.copy()
    plain["out_mask"] = 0
    res0 = gpu.rollout_frontier(plain, fs, n, semantics=N.SEM_ARENA, rng=N.RNG_PHILOX, seed=SEED + 3, root_index=idx)
    assert res.tobytes() == res0.tobytes()
