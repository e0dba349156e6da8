"""Plain CPython restatement of the reference FastMCTSAgent's search, for tests.

The reference search (agents/fast_mcts_agent.py:45-62, 153-186, 243-267) is a bandit
over the root's legal moves: while the root has untried moves an iteration pops the
LAST one and makes it the next child; afterwards every iteration takes the child with
the largest UCB1 value (first child on ties, Python's max()).  The rollout reward is
one number per search, `base`, plus `rng.random() * 0.1`; with an empty cached legal
list (base = NaN here) the reward is 0.0 and no number is drawn.  Reward and visit go
to the chosen child and to the root.

No GPU and no project imports: math and random only.  `rng` is a real random.Random,
so CPython itself is the generator reference (position, lazy twist, 53-bit random()).
"""
import math
import random

TOP = 10


def bandit(n_children, iterations, base, rng, c=1.414):
    """(visits[], totals[]) per child, in child order, after `iterations` iterations on
    a root of n_children legal moves.  len(visits) = children expanded.  Child j was
    expanded from legal[n_children - 1 - j]."""
    visits, totals = [], []
    draw = not math.isnan(base)
    for root_visits in range(iterations):
        if len(visits) < n_children:  # expand: untried_moves.pop()
            visits.append(0)
            totals.append(0.0)
            sel = len(visits) - 1
        else:  # select_child: max() keeps the first of equal values
            two_log = 2 * math.log(root_visits)
            sel, best = 0, -math.inf
            for j in range(len(visits)):
                u = totals[j] / visits[j] + c * (two_log / visits[j]) ** 0.5
                if u > best:
                    sel, best = j, u
        reward = base + rng.random() * 0.1 if draw else 0.0
        visits[sel] += 1
        totals[sel] += reward
    return visits, totals


def summarize(n, iterations, visits, totals):
    """What bk_fastmcts reports for these child statistics (everything but the state)."""
    nch = len(visits)
    assert nch == min(n, iterations)
    best = max(range(nch), key=lambda j: visits[j]) if nch else 0  # first of the most visited
    order = sorted(range(nch), key=lambda j: visits[j], reverse=True)[:TOP]  # stable
    return {
        "iterations": iterations,
        "n_children": nch,
        "best_index": n - 1 - best if nch else 0,
        "n_top": len(order),
        "top_index": [n - 1 - j for j in order],
        "top_visits": [visits[j] for j in order],
        "top_q": [totals[j] / visits[j] for j in order],  # unrounded
        "visits_out": [visits[n - 1 - k] if n - 1 - k < nch else 0 for k in range(n)],
    }


def expected(n, iterations, base, rng, c=1.414):
    """Every field bk_fastmcts returns for one root, plus "state": the 625 words of
    rng (advanced in place) afterwards."""
    visits, totals = bandit(n, iterations, base, rng, c)
    out = summarize(n, iterations, visits, totals)
    out["state"] = list(rng.getstate()[1])
    return out


def rng_at(seed, pos):
    """random.Random(seed) with its position word set to pos (0..624; 624 = a fresh
    generator, which twists before its next word)."""
    r = random.Random(seed)
    words = r.getstate()[1]
    r.setstate((3, tuple(words[:624]) + (pos,), None))
    return r


def round_robin_visits(n, iterations):
    """Closed form for a NaN base: every total stays 0.0, so UCB1 is the exploration term
    alone, equal for equal visits and larger for fewer; first-max ties then visit the
    children in order, round after round.  Child j's visits, for iterations >= n."""
    assert iterations >= n
    return [iterations // n + (j < iterations % n) for j in range(n)]
