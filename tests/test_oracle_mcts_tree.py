"""or_mcts_tree and the fixed-capacity table runs, on the CPU: the referee of
tests/test_gpu_mcts_limits.py is itself pinned here, against or_mcts (which
tests/test_oracle_golden.py pins to the reference) and against the header's sentence on the
table's layout restated in plain Python (tests/search_limits.py).  Tolerance: exact.

CPU time on one core: the golden positions 1.3 s, the small-table runs (3 cases x 16 roots,
plus their large-table twins) 0.2 s."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import search_limits as S
from tests.conftest import load_golden
from tests.helpers import POS, mt_array, replay

MCTS = load_golden("mcts.json")


@pytest.mark.parametrize("case", range(len(MCTS)))
def test_tree_entry_gives_or_mcts_results(case):
    """The positions, seeds and consecutive calls of tests/golden/mcts.json through O.mcts
    and through O.mcts_tree(grow=True): the same results bit for bit, the same table and
    stream; the dump's root children are `children`; visits and totals add up."""
    c = MCTS[case]
    ztab = O.zobrist_table(c["zobrist_seed"])
    boards = [replay(POS[c["position"]]) for _ in range(2)]
    rngs = [O.numpy_mt(c["rollout_seed"]) for _ in range(2)]
    tts = [O.TT() if c["use_tt"] else None for _ in range(2)]
    it = c["iterations"]
    for call in c["calls"]:
        player = call["player"] - 1
        if call["searched"]:
            a = O.mcts(boards[0], player, it, 1.414, c["max_rollout_moves"], ztab, rngs[0], tts[0])
            t = O.mcts_tree(boards[1], player, it, 1.414, c["max_rollout_moves"], ztab, rngs[1], tts[1], grow=True)
            assert t["rc"] == 0 and t["iterations_done"] == it
            assert (t["move"], t["hits"], t["children"]) == (a["move"], a["hits"], a["children"])
            assert t["rewards"].tobytes() == a["rewards"].tobytes()
            assert t["hit_flags"].tobytes() == a["hit_flags"].tobytes()
            assert np.array_equal(mt_array(rngs[0]), mt_array(rngs[1]))
            if c["use_tt"]:
                assert tts[0].count == tts[1].count and S.same_table(tts[1].keys, tts[1].vals, tts[0].keys, tts[0].vals)
                S.check_open_addressing(tts[1].keys, tts[1].vals, tts[1].count)
            check_dump(t, it)
            assert int(t["n_legal"][0]) == call["n_legal"]
        if call["move"] is None:
            break
        for b in boards:
            O.place_move(b, player, call["move"])


def check_dump(t, iterations):
    n = len(t["parent"])
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        p = int(t["parent"][i])
        assert 0 <= p < i  # creation order
        kids[p].append(i)
    assert int(t["parent"][0]) == -1 and int(t["node_move"][0]) == -1
    assert [(int(t["node_move"][i]), int(t["visits"][i]), float(t["total"][i])) for i in kids[0]] == t["children"]
    assert int(t["visits"][0]) == iterations
    total = 0.0
    for r in t["rewards"].tolist():  # left to right, as backpropagation added them
        total += r
    assert float(t["total"][0]) == total
    for i in range(n):
        assert int(t["n_children"][i]) == len(kids[i]) <= int(t["n_legal"][i])
        if int(t["n_legal"][i]) == 0:  # nothing to expand: every visit simulates the node itself again
            assert not kids[i]
        elif i:  # the visit that created it, then one per visit handed on to a child
            assert int(t["visits"][i]) == 1 + sum(int(t["visits"][k]) for k in kids[i]), i
    assert n == 1 + sum(len(k) for k in kids)


@pytest.fixture(scope="module")
def small_runs():
    """{(cap, iterations): [(fixed-cap run, large-cap run)] per 20-ply root}."""
    out = {}
    for cap, iters in S.FULL_CASES + (S.ETT_CASE,):
        runs = []
        for i, b in enumerate(S.ply20_roots()):
            small = S.oracle_search(b, b.cur, iters, S.SMALL_ROLL, S.small_ztab(), S.small_seed(i), S.fixed_tt(cap))
            big = S.oracle_search(b, b.cur, iters, S.SMALL_ROLL, S.small_ztab(), S.small_seed(i), S.fixed_tt(1 << 12))
            runs.append((small, big))
        out[(cap, iters)] = runs
    return out


@pytest.mark.parametrize("case", S.FULL_CASES + (S.ETT_CASE,))
def test_fixed_capacity_tables(small_runs, case):
    cap, iters = case
    wrapped = displaced = refused = 0
    max_disp = 0
    for small, big in small_runs[case]:
        assert big["rc"] == 0
        disp = S.check_open_addressing(small["tt_keys"], small["tt_vals"], small["tt_count"])
        S.check_open_addressing(big["tt_keys"], big["tt_vals"], big["tt_count"])
        k = small["iterations_done"]
        big_keys = big["tt_keys"][~np.isnan(big["tt_vals"])].tolist()
        if small["rc"] == 0:
            assert k == iters
            # the table's size changes no result: the same key set, rewards, tree and stream
            assert sorted(disp) == sorted(big_keys)
            for f in ("rewards", "hit_flags", "parent", "node_move", "visits", "total", "n_children", "n_legal", "mt"):
                assert small[f].tobytes() == big[f].tobytes(), f
            assert (small["move"], small["children"]) == (big["move"], big["children"])
            check_dump(small, iters)
        else:  # one more insert would have left no empty slot
            refused += 1
            assert small["rc"] == -3 and k < iters and small["tt_count"] == cap - 1
            assert set(disp) <= set(big_keys)
            assert small["rewards"][:k].tobytes() == big["rewards"][:k].tobytes()
            assert small["hit_flags"][:k].tobytes() == big["hit_flags"][:k].tobytes()
            # the cap - 1 inserts before it are the first cap - 1 misses of the large-table run
            assert int((big["hit_flags"][:k] == 0).sum()) == cap - 1 and big["hit_flags"][k] == 0
        wrapped += bool(S.wrapped_keys(small["tt_keys"], small["tt_vals"]))
        displaced += any(disp.values())
        max_disp = max(max_disp, max(disp.values()))
    print(case, "searches with wrapped entries", wrapped, "with displaced", displaced, "longest displacement",
          max_disp, "refused", refused)
    # what makes these inputs worth running on the GPU
    assert wrapped >= 12 and displaced == 16 and max_disp >= cap // 2
    if case == S.ETT_CASE:
        assert refused >= 8
    else:
        assert refused == 0
        full = sum(s["tt_count"] == cap - 1 for s, _ in small_runs[case])
        assert full >= 1  # a search with no hit ends with the table as full as it may be


def test_second_search_hits_displaced_and_wrapped_keys(small_runs):
    """The (32, 31) tables searched again from the same root, same iterations: every
    simulation is a hit with the first search's reward, so the second search builds the
    first one's tree again and looks every key of the table up, the displaced ones and the
    ones past the wrap included; the table is left as it was."""
    cap, iters = S.FULL_CASES[0]
    displaced = wrapped = 0
    for i, (b, (first, _)) in enumerate(zip(S.ply20_roots(), small_runs[(cap, iters)])):
        disp = S.check_open_addressing(first["tt_keys"], first["tt_vals"], first["tt_count"])
        tt = S.fixed_tt(cap, first["tt_keys"], first["tt_vals"], first["tt_count"])
        again = S.oracle_search(b, b.cur, iters, S.SMALL_ROLL, S.small_ztab(), S.second_seed(i), tt)
        assert again["rc"] == 0 and again["hit_flags"].all() and again["hits"] == iters
        assert again["rewards"].tobytes() == first["rewards"].tobytes()
        for f in ("parent", "node_move", "visits", "total", "n_children"):
            assert again[f].tobytes() == first[f].tobytes(), f
        assert S.same_table(again["tt_keys"], again["tt_vals"], first["tt_keys"], first["tt_vals"])
        assert np.array_equal(again["mt"], mt_array(O.numpy_mt(S.second_seed(i))))  # no draw
        displaced += sum(d > 0 for d in disp.values())
        wrapped += len(S.wrapped_keys(first["tt_keys"], first["tt_vals"]))
    print("keys hit by the second searches: displaced", displaced, "wrapped", wrapped)
    assert displaced >= 64 and wrapped >= 16
