"""A reference of HeuristicAgent's draw that has no rounding of its own (test infrastructure
only, no GPU).

The HeuristicAgent kernels do not reproduce numpy's softmax bit for bit; they promise that a
draw they certify is the move the reference picks on any host, and that a draw they cannot
certify is flagged ("Exactness").  To test that promise from both sides this
module has:

* features(): (n, corners, edge, anchor_r, anchor_c) of a move, in plain Python from the
  oracle board's grid, from the rule of agents/heuristic_agent.py:68-199 as DESIGN.md 4 states
  it -- written apart from pyoracle.heuristic_score;
* exact_distribution(): the softmax in real arithmetic (stdlib decimal, PREC digits) from the
  double weights: the cumulative ends lo_j, hi_j of every move's interval, in list order;
* double_scores() / numpy_choice(): the reference's own double arithmetic and its own lines
  for the choice (heuristic_agent.py:80-103, :233-244, numpy's rng.choice);
* a Python model of the device's generator cursor {i, mt[i], mt[i + 1], mt[i + 397]}
  (mt_cursor_next, draw_double) and forge_cursor(), which builds a cursor whose next
  random_sample() is a wanted u: bk_arena_advance / bk_arena_step take the seats' cursors from
  the caller, so a draw can be put on an interval end without touching a kernel;
* the positions and the weight sets that tests/test_heuristic_reference.py (CPU) and
  tests/test_gpu_heuristic_draws.py (GPU) share, each computed once per process.
"""
import bisect
import functools
from decimal import Decimal, localcontext

import numpy as np

from oracle import pyoracle as O
from tests import rules_reference as R

PREC = 100                      # decimal digits of the "real" arithmetic
TWO53 = 1 << 53
ULP = Decimal(1) / Decimal(TWO53)  # u = 2^-53 as DESIGN.md 4 writes it
DECIDABLE = Decimal(2) ** -37   # an interval this wide holds draws the kernel must certify

DEFAULT = (1.0, 2.0, -1.5, 0.5)
# twelve sets in three plans of four: the defaults, +-S_max on each single axis
# (S = 5|size| + 20|corner| + 5|edge| + |centre| = 128), one mixed-sign set with S = 128,
# all zero, and one tiny set
WEIGHT_SETS = (
    DEFAULT, (25.6, 0.0, 0.0, 0.0), (-25.6, 0.0, 0.0, 0.0), (0.0, 6.4, 0.0, 0.0),
    (0.0, -6.4, 0.0, 0.0), (0.0, 0.0, 25.6, 0.0), (0.0, 0.0, -25.6, 0.0), (0.0, 0.0, 0.0, 128.0),
    (0.0, 0.0, 0.0, -128.0), (-6.4, 3.2, 3.2, -16.0), (0.0, 0.0, 0.0, 0.0), (1e-300, 1e-300, 1e-300, 1e-300),
)
PLANS = (WEIGHT_SETS[0:4], WEIGHT_SETS[4:8], WEIGHT_SETS[8:12])

# (move count, seed) of O.gen_state: a first move and a second move (short lists, the low end
# of tcr), the earliest board found whose mover has ten decidable moves under every set, the
# last move of the early edge rule and the first of the late one, a one-move board
GEN_POSITIONS = ((1, 1), (6, 1), (13, 3), (29, 1), (30, 3), (52, 4))
# On a board of the first two rounds size = -25.6 leaves at most three moves decidable: a
# piece one cell larger weighs e^-25.6 = 2^-36.9 of the smallest piece's moves, and the mover
# has at most four anchors for its smallest piece.  Such boards are in for their lists, not
# for that count.
EARLY_POSITIONS = ("gen_state(1, 1)", "gen_state(6, 1)")
# (tests/edge_boards.py name, mover)
EDGE_POSITIONS = (("strip_left", 1), ("strip_bottom", 2), ("own_next_to_board_corners", 0))


# ------------------------------------------------------------------------------ features


def _safe_map(board, player):
    """bool[22, 22] (board cell (r, c) at [r + 1, c + 1], False off the board): the cell is
    empty and none of its four edge neighbours is the player's."""
    grid = np.ctypeslib.as_array(board.grid).reshape(20, 20)
    own = np.zeros((22, 22), dtype=bool)
    own[1:21, 1:21] = grid == player + 1
    near = own[:-2, 1:-1] | own[2:, 1:-1] | own[1:-1, :-2] | own[1:-1, 2:]
    safe = np.zeros((22, 22), dtype=bool)
    safe[1:21, 1:21] = (grid == 0) & ~near
    return safe


def features(board, player, move, _safe=None):
    """(n, corners, edge, anchor_r, anchor_c) of move = g * 400 + anchor for player (0..3) on
    the board BEFORE the move: n cells; corners = over the cells, their in-bounds diagonal
    neighbours that are empty and not edge-adjacent to the player (a neighbour of two cells
    counts twice); edge = cells within 2 of the border (the integer count: the callers halve
    it once move_count / 100.0 >= 0.3)."""
    safe = _safe_map(board, player) if _safe is None else _safe
    g, anchor = divmod(int(move), 400)
    ar, ac = divmod(anchor, 20)
    corners = edge = 0
    offsets = R.orients()[g][1]
    for dr, dc in offsets:
        r, c = ar + dr, ac + dc
        corners += int(safe[r, c]) + int(safe[r, c + 2]) + int(safe[r + 2, c]) + int(safe[r + 2, c + 2])
        edge += min(r, c, 19 - r, 19 - c) <= 2
    return len(offsets), corners, int(edge), ar, ac


def features_of(board, player, moves):
    safe = _safe_map(board, player)
    return [features(board, player, m, safe) for m in moves]


# ------------------------------------------------------------------------------ the reference's doubles


def double_scores(feats, move_count, weights=DEFAULT):
    """_evaluate_move's float of each move, accumulated as the reference accumulates it."""
    w_size, w_corner, w_edge, w_centre = weights
    out = []
    for n, corners, edge, ar, ac in feats:
        score = 0.0
        score += w_size * n
        score += w_corner * corners
        edge_score = edge if move_count / 100.0 < 0.3 else edge * 0.5
        score += w_edge * edge_score
        distance = np.sqrt((ar - 9.5) ** 2 + (ac - 9.5) ** 2)
        center = 1.0 - distance / np.sqrt(2 * (9.5 ** 2))
        score += w_centre * center
        out.append(float(score))
    return out


def numpy_cdf(scores):
    x = np.array(scores) / 1.0
    e = np.exp(x - np.max(x))
    p = e / np.sum(e)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    return cdf


def numpy_choice(scores, u):
    """The list index HeuristicAgent picks for random_sample() == u (a float or an array of
    floats): _softmax and the lines of RandomState.choice(n, p=p)."""
    return numpy_cdf(scores).searchsorted(u, side="right")


# ------------------------------------------------------------------------------ real arithmetic


def exact_distribution(feats, move_count, weights):
    """(lo, hi): Decimal lists, the cumulative probability before and after every move in
    list order, for the weights as the doubles they are: score = w . features with
    centre = 1 - sqrt(dr^2 + dc^2) / sqrt(2 * 9.5^2), e = exp(score) (no shift), all at PREC
    digits."""
    with localcontext() as ctx:
        ctx.prec = PREC
        w_size, w_corner, w_edge, w_centre = (Decimal(float(x)) for x in weights)
        late = move_count * 10 >= 300  # move_count / 100.0 >= 0.3
        dmax = (2 * Decimal("9.5") ** 2).sqrt()
        cache = {}
        es = []
        for f in feats:
            e = cache.get(f)
            if e is None:
                n, corners, edge, ar, ac = f
                dr, dc = Decimal(ar) - Decimal("9.5"), Decimal(ac) - Decimal("9.5")
                centre = 1 - (dr * dr + dc * dc).sqrt() / dmax
                edge_score = Decimal(edge) / 2 if late else Decimal(edge)
                e = cache[f] = (w_size * n + w_corner * corners + w_edge * edge_score + w_centre * centre).exp()
            es.append(e)
        total = sum(es)
        lo, hi, run = [], [], Decimal(0)
        for e in es:
            lo.append(run / total)
            run += e
            hi.append(run / total)
        hi[-1] = Decimal(1)
        return lo, hi


def u_decimal(u53):
    """random_sample() == u53 / 2^53 as a Decimal (exact)."""
    with localcontext() as ctx:
        ctx.prec = PREC
        return Decimal(int(u53)) / Decimal(TWO53)


def exact_choice(hi, u53):
    """The first list index whose exact cumulative probability exceeds u."""
    return bisect.bisect_right(hi, u_decimal(u53))


def distance_to_end(lo, hi, u53):
    """(j, d): the exact interval [lo_j, hi_j) that holds u, and u's distance to its nearer end."""
    with localcontext() as ctx:
        ctx.prec = PREC
        u = u_decimal(u53)
        j = bisect.bisect_right(hi, u)
        return j, min(u - lo[j], hi[j] - u)


def to_u53(x, offset=0):
    """The 53-bit draw nearest to the Decimal x, moved by offset draws, clamped to [0, 2^53)."""
    with localcontext() as ctx:
        ctx.prec = PREC
        k = int((x * TWO53).to_integral_value()) + int(offset)
    return min(max(k, 0), TWO53 - 1)


# ------------------------------------------------------------------------------ the device's generator cursor

_M32 = 0xFFFFFFFF


def _init_step(x, j):
    return (1812433253 * (x ^ (x >> 30)) + j) & _M32


def _twist(a, b):
    y = (a & 0x80000000) | (b & 0x7FFFFFFF)
    return (y >> 1) ^ (0x9908B0DF if y & 1 else 0)


def _temper(y):
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    y ^= y >> 18
    return y & _M32


def _untemper(y):
    y ^= y >> 18
    y ^= (y << 15) & 0xEFC60000
    t = y
    for _ in range(5):
        t = y ^ ((t << 7) & 0x9D2C5680)
    y = t & _M32
    t = y
    for _ in range(3):
        t = y ^ (t >> 11)
    return t & _M32


def cursor_init(seed):
    """The cursor of numpy RandomState(seed) before its first output: (i, mt[i], mt[i+1], mt[i+397])."""
    a = int(seed) & _M32
    b = _init_step(a, 1)
    x = b
    for j in range(2, 398):
        x = _init_step(x, j)
    return (0, a, b, x)


def cursor_next(cur):
    """(output, cursor after it): output i = temper(mt[i + 397] ^ twist(mt[i], mt[i + 1])); the
    cursor holds the init_genrand sequence only, so it ends after output 226."""
    i, a, b, c = (int(x) for x in cur)
    if i >= 227:
        raise ValueError("the cursor's 227 outputs are used up")
    v = _temper(c ^ _twist(a, b))
    i += 1
    return v, (i, b, _init_step(b, i + 1), _init_step(c, i + 397))


def random_sample(cur):
    """(u53, cursor after): RandomState.random_sample() == u53 / 2^53, two outputs combined
    as genrand_res53 combines them."""
    x0, cur = cursor_next(cur)
    x1, cur = cursor_next(cur)
    return ((x0 >> 5) << 26) + (x1 >> 6), cur


def _temper_v(y):
    y = y ^ (y >> np.uint32(11))
    y = y ^ ((y << np.uint32(7)) & np.uint32(0x9D2C5680))
    y = y ^ ((y << np.uint32(15)) & np.uint32(0xEFC60000))
    return y ^ (y >> np.uint32(18))


def _init_step_v(x, j):
    return np.uint32(1812433253) * (x ^ (x >> np.uint32(30))) + np.uint32(j)


@functools.lru_cache(maxsize=8)
def _forge_candidates(v0, start, chunk):
    """Cursors (0, 0, b, c) for b in [start, start + chunk) whose first output is
    temper(v0), and their second outputs (kept: neighbouring targets share them)."""
    one, mag, v0 = np.uint32(1), np.uint32(0x9908B0DF), np.uint32(v0)
    b = np.arange(start, start + chunk, dtype=np.uint32)
    y = b & np.uint32(0x7FFFFFFF)
    c = v0 ^ (y >> one) ^ np.where(y & one, mag, np.uint32(0))
    b2 = _init_step_v(b, 2)
    y2 = (b & np.uint32(0x80000000)) | (b2 & np.uint32(0x7FFFFFFF))
    x1 = _temper_v(_init_step_v(c, 398) ^ (y2 >> one) ^ np.where(y2 & one, mag, np.uint32(0)))
    return b, c, x1


def forge_cursor(u53, precision_bits=0):
    """(cursor uint32[4] with i = 0, realised u53): the cursor's next random_sample() has the
    wanted top 27 bits exactly and its low 26 bits within 2^(26 - precision_bits) of the
    wanted ones.  With a = mt[0] = 0 the first output is temper(c ^ twist(0, b)), so c fixes
    it for any b; the second output is a hash of b, searched over b in vectorised chunks.
    Callers classify the realised u, never the wanted one."""
    u53 = int(u53)
    assert 0 <= u53 < TWO53 and 0 <= precision_bits <= 26
    want_lo = u53 & ((1 << 26) - 1)
    v0 = np.uint32(_untemper((u53 >> 26) << 5))
    tol = 1 << (26 - precision_bits)
    chunk = 1 << max(6, min(precision_bits, 17))
    for start in range(0, 1 << 32, chunk):
        b, c, x1 = _forge_candidates(int(v0), start, chunk)
        err = np.abs((x1 >> np.uint32(6)).astype(np.int64) - want_lo)
        k = int(err.argmin())
        if int(err[k]) <= tol:
            cur = (0, 0, int(b[k]), int(c[k]))
            got, _ = random_sample(cur)
            assert got >> 26 == u53 >> 26 and abs(got - u53) <= tol
            return np.array(cur, dtype=np.uint32), got
    raise AssertionError("forge_cursor: no candidate")


# Cursors whose next random_sample() is exactly 1/4, 1/2 and 7/8 (u53 -> cursor): all 26 low
# bits are wanted, one candidate in 2^26, so these were searched once (over b and the five
# free low bits of the first output) and are kept; the model checks them.  With all-zero
# weights every e is 1, the kernel's sums are exact integers, and on a list of n moves with
# n | K 2^53 such a draw lies exactly on the end K / n.
EXACT_CURSORS = {1 << 51: (0, 0, 36932378, 1564086646), 1 << 52: (0, 0, 34119001, 138320060),
                 7 << 50: (0, 0, 12206986, 3897301986)}
ZERO_SET = 10  # WEIGHT_SETS[ZERO_SET] == (0, 0, 0, 0)


# ------------------------------------------------------------------------------ shared inputs


class Position:
    """One board with a mover that has moves: the oracle board with the very tables the
    kernels are given, its packed state and bk_fset record, the legal list in the
    reference's order and its features."""

    def __init__(self, name, board, player):
        from tests.helpers import oracle_fset, pack_many
        self.name, self.board, self.player = name, board, int(player)
        board.cur = self.player
        self.move_count = int(board.move_count)
        self.state = pack_many([board])[0]
        self.fset = oracle_fset(board)
        self.moves = O.legal_moves(board, self.player, O.ORDER_FRONTIER)
        self.feats = features_of(board, self.player, self.moves)
        self.orient = [m // 400 for m in self.moves]
        self.piece = [R.orients()[g][0] for g in self.orient]

    def boundary_kind(self, j):
        """What ends at lo_j (j >= 1): another piece, another orientation, or neither."""
        if self.piece[j] != self.piece[j - 1]:
            return "piece"
        return "orientation" if self.orient[j] != self.orient[j - 1] else "anchor"


@functools.lru_cache(maxsize=None)
def positions():
    from tests import edge_boards as E
    out = []
    for m, s in GEN_POSITIONS:
        b = O.gen_state(m, s)[0]
        out.append(Position(f"gen_state({m}, {s})", b, b.cur))
    names = E.edge_names()
    for name, mover in EDGE_POSITIONS:
        b = O.copy_board(E.edge_boards()[names.index(name)])
        out.append(Position(name, b, mover))
    return tuple(out)


class Pair:
    """A (position, weight set): the exact intervals, the reference's doubles, and the
    placements the tests put draws on."""

    def __init__(self, pos, set_index):
        self.pos, self.set_index = pos, set_index
        self.weights = WEIGHT_SETS[set_index]
        self.lo, self.hi = exact_distribution(pos.feats, pos.move_count, self.weights)
        self.scores = double_scores(pos.feats, pos.move_count, self.weights)
        self.cdf = numpy_cdf(self.scores)
        n = len(pos.moves)
        self.decidable = [j for j in range(n) if self.hi[j] - self.lo[j] >= DECIDABLE]
        self.tested_moves = self._spread_moves(24)
        self.tested_boundaries = self._spread_boundaries(12)

    def _spread_moves(self, cap):
        """Up to cap decidable moves: the first and the last, the decidable moves on both sides
        of every piece and orientation boundary between two of them, the rest spread evenly."""
        dec, pos = self.decidable, self.pos
        if len(dec) <= cap:
            return list(dec)
        must = [dec[0], dec[-1]]
        for a, b in zip(dec, dec[1:]):
            if b == a + 1 and pos.boundary_kind(b) != "anchor":
                must += [a, b]
        must = sorted(set(must))
        if len(must) > cap:  # keep the ends, thin the rest evenly
            keep = np.linspace(0, len(must) - 1, cap).round().astype(int)
            return sorted({must[k] for k in keep})
        rest = [j for j in dec if j not in set(must)]
        extra = np.linspace(0, len(rest) - 1, cap - len(must)).round().astype(int) if rest else []
        return sorted(set(must) | {rest[k] for k in extra})

    def _spread_boundaries(self, cap):
        """Up to cap interval ends lo_j (j >= 1): a third each of piece boundaries, orientation
        boundaries and ends between two anchors, those that touch a decidable move, spread
        over the list; where no boundary of a kind touches one, the first two of that kind."""
        dec, pos = set(self.decidable), self.pos
        every = range(1, len(pos.moves))
        out = []
        for kind in ("piece", "orientation", "anchor"):
            room = cap // 3 if kind != "anchor" else cap - len(out)
            js = [j for j in every if pos.boundary_kind(j) == kind and (j in dec or j - 1 in dec)]
            if not js:
                js = [j for j in every if pos.boundary_kind(j) == kind][:2]
            if len(js) > room:
                js = [js[i] for i in sorted(set(np.linspace(0, len(js) - 1, room).round().astype(int)))]
            out += js
        return sorted(out)


@functools.lru_cache(maxsize=None)
def pairs():
    """Every (position, weight set), position-major."""
    return tuple(Pair(p, s) for p in positions() for s in range(len(WEIGHT_SETS)))


# ------------------------------------------------------------------------------ full games at the bound

# four sets with S = 128, rotated over the seats of eight arena games from the empty board
FULL_SETS = ((-6.4, 3.2, 3.2, -16.0), (0.0, 0.0, -25.6, 0.0), (0.0, 6.4, 0.0, 0.0), (0.0, 0.0, 0.0, 128.0))
FULL_GAMES = 8
FULL_SEED0 = 61000


def full_game_seeds(i):
    return [FULL_SEED0 + 10 * i + p for p in range(4)]


def full_game_seat_sets(i):
    """Seat p of game i plays FULL_SETS[(p + i) % 4]."""
    return [(p + i) & 3 for p in range(4)]


def full_game_referee(i):
    """Game i by the arena loop with the reference's doubles (pyoracle.mixed_playout_arena's
    loop), every draw also classified in real arithmetic: ((scores, winner_mask, plies,
    passes, turns), [(numpy index, exact index, d) per placement])."""
    b = O.new_board()
    rngs = [np.random.RandomState(s) for s in full_game_seeds(i)]
    sets = [FULL_SETS[k] for k in full_game_seat_sets(i)]
    draws, passes, turns, plies = [], 0, 0, 0
    while turns < 2500:
        lists = [O.legal_moves(b, p, O.ORDER_FRONTIER) for p in range(4)]
        if not any(lists):
            break
        p = b.cur
        turns += 1
        moves = lists[p]
        if not moves:
            passes += 1
            b.cur = (b.cur + 1) & 3
            continue
        feats = features_of(b, p, moves)
        u = rngs[p].random_sample()
        u53 = int(u * TWO53)
        assert u53 / TWO53 == u
        k = int(numpy_choice(double_scores(feats, b.move_count, sets[p]), u))
        lo, hi = exact_distribution(feats, b.move_count, sets[p])
        j, d = distance_to_end(lo, hi, u53)
        draws.append((k, j, d))
        O.place_move(b, p, moves[k])
        b.cur = (p + 1) & 3
        plies += 1
    scores, wm = O.game_scores(b)
    return (list(scores), wm, plies, passes, turns), draws
