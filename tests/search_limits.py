"""Shared by tests/test_oracle_mcts_tree.py (CPU) and tests/test_gpu_mcts_limits.py: the
open-addressing checker, the small-table inputs and the fixed-capacity oracle runs, the
late roots with few legal moves, and plain-Python walks over a returned node pool."""
import ctypes as C
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import pyoracle as O
from tests.helpers import mt_array

EXPLORATION = 1.414

# ------------------------------------------------------------------ the header's TT sentence


def check_open_addressing(keys, vals, count):
    """include/blokus_hip.h: "open addressing (linear probing, slot = key & (tt_cap - 1),
    empty slot = NaN value), tt_count[g] entries".  Every live key is found by probing from
    its home slot with no empty slot on the way, count is the number of live slots, no key
    is stored twice, and one slot at least is empty (else a probe for an absent key never
    ends).  Returns {key: displacement from the home slot}."""
    cap = len(keys)
    assert cap >= 2 and cap & (cap - 1) == 0 and len(vals) == cap
    live = [i for i in range(cap) if not math.isnan(float(vals[i]))]
    assert len(live) == int(count), (len(live), int(count))
    assert len(live) < cap
    disp = {}
    for i in live:
        key = int(keys[i])
        assert key not in disp, key
        j, steps = key & (cap - 1), 0
        while j != i:
            assert not math.isnan(float(vals[j])), (key, i, j)
            assert int(keys[j]) != key
            j, steps = (j + 1) & (cap - 1), steps + 1
        disp[key] = steps
    return disp


def wrapped_keys(keys, vals):
    """Live keys stored below their home slot: their probe went past the table's end."""
    cap = len(keys)
    return [int(keys[i]) for i in range(cap)
            if not math.isnan(float(vals[i])) and i < (int(keys[i]) & (cap - 1))]


def same_table(keys, vals, want_keys, want_vals):
    """Slot for slot: the same slots empty (NaN), the same key and value bits in the others."""
    keys, vals, want_keys, want_vals = (np.asarray(x) for x in (keys, vals, want_keys, want_vals))
    live = ~np.isnan(want_vals)
    return (np.array_equal(np.isnan(vals), ~live) and np.array_equal(keys[live], want_keys[live]) and
            np.array_equal(vals[live].view(np.uint64), want_vals[live].view(np.uint64)))


# ------------------------------------------------------------------ oracle runs


def zobrist_hash(b, ztab):
    return int(O.lib().or_zobrist_hash(C.byref(b), ztab.ctypes.data_as(C.POINTER(C.c_uint64))))


def fixed_tt(cap, keys=None, vals=None, count=0):
    tt = O.TT(cap)
    if keys is not None:
        tt.keys[:], tt.vals[:], tt.count = keys, vals, int(count)
    return tt


def oracle_search(b, player, iterations, roll, ztab, seed, tt, heuristic=False, grow=False, mt=None):
    """One or_mcts_tree search from numpy seed `seed` (or the MT `mt`, advanced): the
    wrapper's dict plus 'mt' (the stream's state after, bk_mcts's layout) and copies of the
    table after the search ('tt_keys', 'tt_vals', 'tt_count')."""
    m = O.numpy_mt(seed) if mt is None else mt
    r = O.mcts_tree(b, player, iterations, EXPLORATION, roll, ztab, m, tt, heuristic=heuristic, grow=grow)
    r["mt"] = mt_array(m)
    if tt is not None:
        r.update(tt_keys=tt.keys.copy(), tt_vals=tt.vals.copy(), tt_count=tt.count)
    return r


def pool16(fn, items):
    """fn over items on 16 threads (ctypes releases the GIL; the oracle's rollout policy is
    thread-local and every call sets its own)."""
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(fn, items))


# ------------------------------------------------------------------ small-table inputs

SMALL_ROLL = 6
SMALL_ZOBRIST_SEED = 5
FULL_CASES = ((32, 31), (64, 63))    # the table ends as full as it may where no iteration hits
TINY_CASES = ((2, 1), (4, 3))        # the smallest legal tables
ETT_CASE = (32, 40)                  # the insert that would fill the last slot is refused


@functools.lru_cache(maxsize=None)
def ply20_roots():
    """16 roots of exactly 20 plies."""
    return tuple(O.gen_state(20, 320 + i)[0] for i in range(16))


def small_seed(i):
    return 40 + i


def second_seed(i):
    """The stream of root i's second search of the same table."""
    return 140 + i


@functools.lru_cache(maxsize=None)
def small_ztab():
    z = O.zobrist_table(SMALL_ZOBRIST_SEED)
    z.setflags(write=False)
    return z


# ------------------------------------------------------------------ late roots

LATE_CLASSES = (0, 1, 2, 3, 4, 5)
LATE_PER_CLASS = 4
LATE_MORE = 16


LATE_SEED0, LATE_LO, LATE_HI, LATE_BOARDS = 4400, 36, 60, 400


def late_board_players():
    """(board, mover, legal count) over the board-players of oracle_states(400, seed0=4400,
    lo=36, hi=60), in order, one board at a time (of its 1,600 board-players 331 have no
    move, 55 one, 49 two, 41 three, 42 four and 34 five: a few dozen boards fill the classes)."""
    rng = np.random.RandomState(LATE_SEED0)  # oracle_states's own sequence
    for i in range(LATE_BOARDS):
        b, _ = O.gen_state(int(rng.randint(LATE_LO, LATE_HI + 1)), LATE_SEED0 + i)
        for p in range(4):
            yield b, p, len(O.legal_moves(b, p))


def with_mover(b, p):
    """A copy of board b with p to move (as edge_boards.search_roots sets the mover)."""
    c = O.copy_board(b)
    c.cur = p
    return c


@functools.lru_cache(maxsize=None)
def late_roots():
    """[(board with the mover set, mover, legal count)]: the first LATE_PER_CLASS
    board-players with 0, 1, 2, 3, 4 and 5 legal moves each, then the first LATE_MORE with
    more than 5, interleaved so that neighbours in a launch differ."""
    groups = [[] for _ in range(len(LATE_CLASSES) + 1)]
    want = [LATE_PER_CLASS] * len(LATE_CLASSES) + [LATE_MORE]
    for x in late_board_players():
        k = min(x[2], len(LATE_CLASSES))
        if len(groups[k]) < want[k]:
            groups[k].append(x)
            if [len(g) for g in groups] == want:
                break
    assert [len(g) for g in groups] == want
    picked = []
    for j in range(max(len(g) for g in groups)):
        picked += [g[j] for g in groups if j < len(g)]
    return tuple((with_mover(b, p), p, n) for b, p, n in picked)


# ------------------------------------------------------------------ node pools


def block_slots(n_exp, n_legal):
    """Slots the header's rule hands a node with n_exp children of n_legal legal moves:
    min(4, L) at the first expansion, then a block twice as large (capped at L) each time
    the block is full."""
    if n_exp == 0:
        return 0
    size = min(4, n_legal)
    total = size
    while size < n_exp:
        size = min(2 * size, n_legal)
        total += size
    return total


def walk_pool(pool, nodes_used):
    """The tree in bk_mcts_node pool `pool` by paths of child indices: {path: slot}, after
    asserting that every child block lies inside [1, nodes_used) and that no two blocks
    overlap, and the slots the header's growth rule needs for this tree."""
    tree, blocks, need = {}, [], 1
    stack = [((), 0)]
    while stack:
        path, i = stack.pop()
        nd = pool[i]
        tree[path] = i
        ne = int(nd["n_exp"])
        if ne:
            c0 = int(nd["child0"])
            assert 1 <= c0 and c0 + ne <= nodes_used, (path, c0, ne, nodes_used)
            blocks.append((c0, c0 + ne))
            need += block_slots(ne, int(nd["n_legal"]))
            stack += [(path + (k,), c0 + k) for k in range(ne)]
        else:
            assert int(nd["child0"]) == -1, (path, int(nd["child0"]))
    blocks.sort()
    for (_, e0), (s1, _) in zip(blocks, blocks[1:]):
        assert e0 <= s1, blocks
    return tree, need


def oracle_paths(r):
    """or_mcts_tree's dump by the same paths: {path: node index}."""
    kids = {}
    for i, p in enumerate(r["parent"].tolist()):
        if p >= 0:
            kids.setdefault(p, []).append(i)  # creation order = expansion order
    paths, stack = {}, [((), 0)]
    while stack:
        path, i = stack.pop()
        paths[path] = i
        stack += [(path + (k,), c) for k, c in enumerate(kids.get(i, []))]
    assert len(paths) == len(r["parent"])
    return paths
