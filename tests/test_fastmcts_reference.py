"""tests/fastmcts_reference.py (the plain restatement the GPU tests of k_fastmcts compare
with) is the reference's search: it reproduces the recorded FastMCTSAgent.think results
of tests/golden/fastmcts.json, and its NaN-base behaviour has a closed form.
Tolerance: exact (moves, visits, Q rounded to 4 places as the reference records it)."""
import math
import random

from oracle import pyoracle as O
from tests import fastmcts_reference as R
from tests.conftest import load_golden
from tests.helpers import POS, replay

FAST = [r for r in load_golden("fastmcts.json") if r["iterations"] <= 600]


def quick_base(legal, pid_of):
    """_fast_rollout's reward before the noise (fast_mcts_agent.py:260-277) of move ints
    g * 400 + row * 20 + col: first 3 by piece id descending (stable), nearest the centre."""
    def dist(m):
        return abs(m % 400 // 20 - 9.5) + abs(m % 20 - 9.5)
    by_size = sorted(legal, key=lambda m: pid_of[m // 400], reverse=True)
    q = sorted(by_size[:3], key=dist)[0]
    return pid_of[q // 400] * 0.1 + (20 - dist(q)) * 0.05


def test_restatement_reproduces_reference_records():
    assert len(FAST) == 32
    pid_of = [pid for pid, _, _ in O.orient_table()]
    for rec in FAST:
        b = replay(POS[rec["position"]])
        legal = O.legal_moves(b, b.cur)
        n, iters = len(legal), rec["iterations"]
        assert n == rec["n_legal"]
        e = R.expected(n, iters, quick_base(legal, pid_of), random.Random(rec["seed"]))
        assert iters >= 5  # below that think() returns the quick move instead
        assert legal[e["best_index"]] == rec["move"], rec
        assert max(e["iterations"], 1) == rec["nodes"], rec
        top = [[legal[i], v, round(q, 4)] for i, v, q in zip(e["top_index"], e["top_visits"], e["top_q"])]
        assert top == rec["top"], rec
        assert sum(e["visits_out"]) == iters


def test_nan_base_is_round_robin():
    for n, iters in [(1, 1), (1, 7), (2, 5), (3, 3), (64, 64 * 5 + 17), (65, 65 * 5 + 17), (129, 129 * 5 + 17),
                     (500, 1100)]:
        rng = R.rng_at(n, 624)
        before = rng.getstate()
        visits, totals = R.bandit(n, iters, math.nan, rng)
        assert visits == R.round_robin_visits(n, iters), (n, iters)
        assert totals == [0.0] * n
        assert rng.getstate() == before  # no draw


def test_rng_at_sets_only_the_position():
    words = random.Random(9).getstate()[1]
    for pos in (0, 1, 623, 624):
        assert R.rng_at(9, pos).getstate() == (3, words[:624] + (pos,), None)
    r = R.rng_at(9, 623)  # the next random() straddles the twist
    r.random()
    assert r.getstate()[1][624] == 1
