#!/usr/bin/env python3
"""CPU replay: how many wave iterations of k_rollout_fr go to learning that a player is
stuck, and how many of them idle lanes could take over.

The kernel's iteration is wave-wide: one derive + movegen pass for the mover of every lane
that has a game.  A lane spends one iteration per placement and one per *discovery* (the
first time a player's turn comes and it has no move; later turns of that player are skipped
without an iteration).  A wave runs until its longest lane is through.

Helper scheme replayed here (the kernel's rule): lanes without a game are helpers, in lane
order; helper k looks at client k // 3 (clients in lane order) and that client's
(k % 3 + 1)-th player after the mover that is not yet known to be stuck, on the client's
board at the top of the iteration.  A player found stuck is skipped at its turn without an
iteration (stuck players stay stuck).

The stencil skips an orientation whose piece no lane of the wave may still play, so a
helper's player adds its free pieces to that union.  The stencil cost of an iteration is
counted as the anchor rows (21 - height) of the orientations in the union.  A variant is
counted next to it (not built: it saves nothing): a helper asks about the smallest pieces
only -- a legal placement of a piece contains, around the frontier cell it covers, a legal
placement of every smaller connected shape, so a player that holds the monomino is stuck
iff the monomino does not fit, else the same with the domino, else with the two trominoes
if it holds both.

Waves of 64 playouts (one game per lane) of one root each; the roots are the oracle's
frontier-order Philox positions after --root-plies placements, as the benchmark's.

  python tools/replay_pass_helpers.py [--roots 12] [--waves-per-root 4] [--root-plies 20]
"""
from __future__ import annotations

import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyoracle as O  # noqa: E402

WAVE = 64


def stuck(b, q):
    return not O.legal_moves(b, q, O.ORDER_FRONTIER)


_W = None


def piece_weights():
    """anchor rows of the stencil per piece (bit = piece id - 1), summed over its orientations"""
    global _W
    if _W is None:
        _W = [0] * 21
        for piece, _, cells in O.orient_table():
            _W[piece - 1] += 21 - (max(r for r, _ in cells) + 1)
    return _W


def stencil_rows(union):
    return sum(w for i, w in enumerate(piece_weights()) if (union >> i) & 1)


def small_pieces(avail):
    """the pieces that decide whether a player with these free pieces is stuck"""
    if avail & 1:
        return 1
    if avail & 2:
        return 2
    if avail & 0xC == 0xC:
        return 0xC
    return avail


def game(root, seed, pid):
    """One playout: (movers of its placements in order, root mover, stuck_at[q] = number of
    placements after which q first has no move, pieces of the placements, used masks at the root)."""
    b = O.copy_board(root)
    _, tr = O.playout_arena_philox(b, seed, pid, O.ORDER_FRONTIER)
    w = O.copy_board(root)
    cur0 = cur = w.cur
    boards, movers, pieces = [O.copy_board(w)], [], []
    used0 = list(O.pack(w).used)
    orients = O.orient_table()
    for mv in tr:
        if mv >= 0:
            O.place_move(w, cur, mv)
            movers.append(cur)
            pieces.append(orients[mv // 400][0] - 1)
            boards.append(O.copy_board(w))
        cur = (cur + 1) & 3
    n = len(movers)
    stuck_at = []
    for q in range(4):
        last = max((i + 1 for i, m in enumerate(movers) if m == q), default=0)
        lo, hi = last, n  # stuck on boards[hi] (the game is over there), monotone in between
        assert stuck(boards[n], q)
        while lo < hi:
            mid = (lo + hi) // 2
            if stuck(boards[mid], q):
                hi = mid
            else:
                lo = mid + 1
        stuck_at.append(lo)
    return movers, cur0, stuck_at, pieces, used0


class Lane:
    def __init__(self, g):
        self.movers, self.cur, self.stuck_at, self.pieces, used0 = g
        self.used = list(used0)
        self.t = 0          # placements made
        self.out = 0        # players skipped or discovered at their turn
        self.known = 0      # players a helper found stuck
        self.done = False
        self.iters = 0
        self.disc = 0       # discoveries paid with an iteration

    def top(self):
        """the kernel's skip loop; True if the lane still has a game"""
        while not self.done:
            if self.out == 0xF:
                self.done = True
            elif ((self.out | self.known) >> self.cur) & 1:
                self.out |= 1 << self.cur
                self.cur = (self.cur + 1) & 3
            else:
                break
        return not self.done

    def avail(self, q):
        return ~self.used[q] & 0x1FFFFF

    def wanted(self, k):
        """the k-th (1..3) player after the mover not yet known stuck, or None"""
        for d in (1, 2, 3):
            q = (self.cur + d) & 3
            if not ((self.out | self.known) >> q) & 1:
                k -= 1
                if k == 0:
                    return q
        return None

    def step(self):
        self.iters += 1
        if self.stuck_at[self.cur] <= self.t:
            self.out |= 1 << self.cur
            self.disc += 1
        else:
            assert self.movers[self.t] == self.cur
            self.used[self.cur] |= 1 << self.pieces[self.t]
            self.t += 1
        self.cur = (self.cur + 1) & 3


def run_wave(games, helpers, small=True):
    lanes = [Lane(g) for g in games]
    iters = helped = helper_slots = rows = pure = 0
    while True:
        clients = [ln for ln in lanes if ln.top()]
        if not clients:
            break
        iters += 1
        found = []
        union = 0
        for c in clients:
            union |= c.avail(c.cur)
        if helpers:
            idle = len(lanes) - len(clients)
            for k in range(min(idle, 3 * len(clients))):
                c = clients[k // 3]
                q = c.wanted(k % 3 + 1)
                if q is not None:
                    helper_slots += 1
                    union |= small_pieces(c.avail(q)) if small else c.avail(q)
                    if c.stuck_at[q] <= c.t:
                        found.append((c, q))
        pure += all(c.stuck_at[c.cur] <= c.t for c in clients)  # no lane places: no locate, no set ops
        for c in clients:
            c.step()
        for c, q in found:
            helped += not (c.known >> q) & 1
            c.known |= 1 << q
        rows += stencil_rows(union)
    return iters, lanes, helped, helper_slots, rows, pure


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--roots", type=int, default=12)
    ap.add_argument("--waves-per-root", type=int, default=4)
    ap.add_argument("--root-plies", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    O.lib()
    roots = []
    for r in range(a.roots):
        b = O.new_board()
        O.playout_arena_philox(b, a.seed, r, O.ORDER_FRONTIER, max_plies=a.root_plies)
        roots.append(b)
    jobs = [(r, w * WAVE + i) for r in range(a.roots) for w in range(a.waves_per_root) for i in range(WAVE)]
    with ThreadPoolExecutor(a.threads) as ex:
        games = list(ex.map(lambda j: game(roots[j[0]], a.seed + 1 + j[0], j[1]), jobs))
    waves = [games[i:i + WAVE] for i in range(0, len(games), WAVE)]
    base = [run_wave(w, False) for w in waves]
    full = [run_wave(w, True, small=False) for w in waves]
    new = [run_wave(w, True) for w in waves]
    nl = len(games)
    placements = sum(len(g[0]) for g in games)
    it0, it1 = sum(x[0] for x in base), sum(x[0] for x in new)
    li0 = sum(ln.iters for x in base for ln in x[1])
    li1 = sum(ln.iters for x in new for ln in x[1])
    d0 = sum(ln.disc for x in base for ln in x[1])
    d1 = sum(ln.disc for x in new for ln in x[1])
    for x, y in zip(base, new):  # the games themselves do not change
        assert [ln.t for ln in x[1]] == [ln.t for ln in y[1]]
    print(f"roots {a.roots} ({a.root_plies} plies), waves {len(waves)}, games {nl}")
    print(f"mean placements per game           {placements / nl:8.2f}")
    print(f"mean lane iterations    today      {li0 / nl:8.2f}   with helpers {li1 / nl:8.2f}")
    print(f"mean discoveries / game today      {d0 / nl:8.2f}   with helpers {d1 / nl:8.2f}"
          f"   ({100.0 * (d0 - d1) / d0:.1f} % taken over by helpers)")
    print(f"mean wave iterations    today      {it0 / len(waves):8.2f}   with helpers {it1 / len(waves):8.2f}"
          f"   ({100.0 * (it0 - it1) / it0:.2f} % fewer)")
    p0, p1 = sum(x[5] for x in base) / len(waves), sum(x[5] for x in new) / len(waves)
    print(f"  of them with no placement today      {p0:8.2f}   with helpers {p1:8.2f}"
          f"   (such an iteration runs the stencil alone: the iterations saved are of this cheap kind)")
    print(f"idle lane-iterations    today      {100.0 * (1 - li0 / (WAVE * it0)):8.2f} %")
    print(f"helper lane-iterations with a pair {sum(x[3] for x in new) / len(waves):8.1f} per wave,"
          f" {sum(x[2] for x in new) / len(waves):.1f} of them find a stuck player first")
    r0, rf, r1 = (sum(x[4] for x in v) / len(waves) for v in (base, full, new))
    print(f"stencil anchor rows per wave (orientations of the pieces some lane may play, all iterations):")
    print(f"    today {r0:9.0f}   helpers, all their pieces {rf:9.0f} ({100.0 * (rf - r0) / r0:+.2f} %)"
          f"   helpers, smallest pieces {r1:9.0f} ({100.0 * (r1 - r0) / r0:+.2f} %)")
    print(f"    per iteration: today {r0 * len(waves) / it0:7.1f}   all pieces {rf * len(waves) / it1:7.1f}"
          f"   smallest pieces {r1 * len(waves) / it1:7.1f}   (all 91 orientations: {stencil_rows(0x1FFFFF)})")
    per = sorted(100.0 * (x[0] - y[0]) / x[0] for x, y in zip(base, new))
    print(f"per-wave cut: min {per[0]:.2f} %  median {per[len(per) // 2]:.2f} %  max {per[-1]:.2f} %")


if __name__ == "__main__":
    main()
