"""tests/heuristic_reference.py against what it restates (CPU only): the cursor model
against numpy's RandomState, the forged cursors against the model, the features and the
double accumulation against the reference's recorded scores (tests/golden/heuristic.json,
heuristic_weights.json), the reference's own doubles against the real-arithmetic softmax on
the inputs of tests/test_gpu_heuristic_draws.py, and those inputs against the situations
they are there for.  Where a comparison of the numpy replay with the exact intervals fails
here, the GPU test's inputs are wrong, not a kernel."""
from decimal import Decimal

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from tests import heuristic_reference as H
from tests.conftest import load_golden
from tests.helpers import POS, replay, sha_ints

SEEDS = (0, 1, 5489, 20260311, 2**31, 2**32 - 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_cursor_model_equals_randomstate(seed):
    """random_sample() of the cursor model is RandomState(seed).random_sample() for the first
    113 samples, the cursor's 226 outputs (+ one); the next sample is refused."""
    want = np.random.RandomState(seed).random_sample(113)
    cur = H.cursor_init(seed)
    for k in range(113):
        u53, cur = H.random_sample(cur)
        assert u53 / 2.0**53 == want[k], (seed, k)
    assert cur[0] == 226
    with pytest.raises(ValueError):
        H.random_sample(cur)


@pytest.mark.parametrize("precision_bits", [0, 14, 18, 20])
def test_forged_cursor_yields_the_draw_it_reports(precision_bits):
    rng = np.random.RandomState(precision_bits)
    targets = [0, 1, (1 << 26) - 1, 1 << 26, H.TWO53 - 1, H.TWO53 - (1 << 26)]
    targets += [int(x) for x in rng.randint(0, H.TWO53, size=8, dtype=np.int64)]
    for want in targets:
        cur, got = H.forge_cursor(want, precision_bits)
        assert cur.dtype == np.uint32 and cur.shape == (4,) and cur[0] == 0
        u53, after = H.random_sample(tuple(int(x) for x in cur))
        assert u53 == got and after[0] == 2
        assert got >> 26 == want >> 26 and abs(got - want) <= 1 << (26 - precision_bits), (want, got)


def test_features_reproduce_the_recorded_default_scores():
    """features + double_scores give the reference's _evaluate_move floats of heuristic.json
    bit for bit (every case by its hash, the listed ones value by value)."""
    import hashlib
    from oracle import pyoracle as O
    for c in load_golden("heuristic.json")["cases"]:
        b = replay(POS[c["position"]])
        p = c["player"] - 1
        moves = O.legal_moves(b, p, O.ORDER_FRONTIER)
        assert sha_ints(moves) == c["moves_sha"]
        got = [x.hex() for x in H.double_scores(H.features_of(b, p, moves), b.move_count)]
        assert hashlib.sha256(",".join(got).encode()).hexdigest() == c["scores_sha"], c["position"]
        if "scores" in c:
            assert got == c["scores"]


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_features_reproduce_the_recorded_weighted_scores(name):
    """The same with the reference's weight sets A to D, under both edge rules."""
    fx = load_golden("heuristic_weights.json")
    w = N.heur_weight_set(fx["weight_sets"][name])
    counts = set()
    for c in fx["scores"]:
        b = replay(POS[c["position"]])
        assert b.move_count == c["move_count"]
        counts.add(b.move_count >= 30)
        got = H.double_scores(H.features_of(b, c["player"] - 1, c["moves"]), b.move_count, w)
        assert [x.hex() for x in got] == c["scores"][name], c["position"]
    assert counts == {False, True}


def test_pyoracle_weights_argument():
    """pyoracle.heuristic_score with weights is the double accumulation here; without, and
    with the defaults, it is the float it was."""
    from oracle import pyoracle as O
    for pos in H.positions()[:5]:
        some = pos.moves[::7]
        feats = [pos.feats[j] for j in range(0, len(pos.moves), 7)]
        for w in (None,) + H.WEIGHT_SETS:
            got = [O.heuristic_score(pos.board, pos.player, m, w) for m in some] if w is not None else \
                [O.heuristic_score(pos.board, pos.player, m) for m in some]
            want = H.double_scores(feats, pos.move_count, H.DEFAULT if w is None else w)
            assert [float(x).hex() for x in got] == [x.hex() for x in want], (pos.name, w)


@pytest.mark.parametrize("k", range(len(H.GEN_POSITIONS) + len(H.EDGE_POSITIONS)))
def test_reference_alone_is_inside_the_property(k):
    """On every (position, set) the numpy replay on this host agrees with real arithmetic
    where the kernels are asked to: its cumulative probabilities are within 2^-45 of the exact
    ends (measured: below 2^-48), and for u = lo_j +- 2^-39 of every move j it picks the
    exact index."""
    worst = Decimal(0)
    for pair in H.pairs()[k * len(H.WEIGHT_SETS):(k + 1) * len(H.WEIGHT_SETS)]:
        err = max(abs(Decimal(float(c)) - h) for c, h in zip(pair.cdf, pair.hi))
        worst = max(worst, err)
        assert err < Decimal(2) ** -45, (pair.pos.name, pair.weights, err)
        u53 = sorted({H.to_u53(x, d) for x in pair.lo for d in (-(1 << 14), 1 << 14)})
        us = np.array(u53, dtype=np.float64) / 2.0**53
        got = np.asarray(H.numpy_choice(pair.scores, us))
        want = [H.exact_choice(pair.hi, x) for x in u53]
        assert got.tolist() == want, (pair.pos.name, pair.weights)
    print("largest |numpy cdf - exact| in units of 2^-45:", float(worst * 2**45))


def test_zero_weights_are_uniform():
    """All-zero weights: hi_j = (j + 1) / n exactly, the choice is floor(u n)."""
    for pair in H.pairs():
        if pair.set_index != 10:
            continue
        n = len(pair.pos.moves)
        assert all(h * n == j + 1 for j, h in enumerate(pair.hi))
        for u53 in (0, 1, H.TWO53 // 3, H.TWO53 - 1):
            assert H.exact_choice(pair.hi, u53) == (u53 * n) >> 53


def test_inputs_contain_their_situation():
    """The positions and sets cover what they were chosen for."""
    pos, pairs = H.positions(), H.pairs()
    assert len(pos) == 9 and len(H.WEIGHT_SETS) == 12 and len(pairs) == 108
    for w in H.WEIGHT_SETS:
        assert N.heur_weight_span(w) <= N.HEUR_MAX_S
    assert sum(N.heur_weight_span(w) == N.HEUR_MAX_S for w in H.WEIGHT_SETS) == 9  # on the bound itself
    assert {29, 30} <= {p.move_count for p in pos}  # both planes of ta
    feats = [(p, f) for p in pos for f in p.feats]
    assert any(p.move_count >= 30 and f[2] % 2 == 1 for p, f in feats)  # edge * 0.5 with an odd count
    assert any(p.move_count >= 30 and f[2] == 5 for p, f in feats) and any(f[2] == 0 for _, f in feats)
    assert any(f[1] == 0 for _, f in feats) and any(f[1] >= 12 for _, f in feats)  # tcr's ends
    assert {f[0] for _, f in feats} == {1, 2, 3, 4, 5}
    quadrants = {(f[3] < 10, f[4] < 10) for _, f in feats}
    assert len(quadrants) == 4
    assert {9, 10} <= {f[3] for _, f in feats} and {9, 10} <= {f[4] for _, f in feats}
    # rows and columns on either side of 9.5 at unequal distance, so that ir and ic of tct are told apart
    assert any(abs(f[3] - 9.5) != abs(f[4] - 9.5) for _, f in feats)
    one = [p for p in pos if len(p.moves) == 1]
    assert len(one) == 1
    for p in pos:  # list order: piece ascending, orientation ascending
        assert p.orient == sorted(p.orient) and p.piece == sorted(p.piece)
    for pair in pairs:
        if len(pair.pos.moves) == 1:
            assert pair.decidable == [0] and not pair.tested_boundaries
            continue
        if pair.pos.name not in H.EARLY_POSITIONS:
            assert len(pair.decidable) >= 10, (pair.pos.name, pair.weights, len(pair.decidable))
        assert 2 <= len(pair.tested_moves) <= 24 and set(pair.tested_moves) <= set(pair.decidable)
        assert pair.decidable[0] in pair.tested_moves and pair.decidable[-1] in pair.tested_moves
        kinds = {pair.pos.boundary_kind(j) for j in pair.tested_boundaries}
        assert {"piece", "orientation"} <= kinds, (pair.pos.name, pair.weights, kinds)
        assert len(pair.tested_boundaries) <= 12
    # somewhere a decidable move sits on each side of a piece boundary and of an orientation boundary
    for kind in ("piece", "orientation"):
        assert sum(1 for pair in pairs for j in pair.tested_boundaries
                   if pair.pos.boundary_kind(j) == kind and j in pair.tested_moves and j - 1 in pair.tested_moves) >= 20


@pytest.mark.parametrize("game", range(H.FULL_GAMES))
def test_full_game_referee_agrees_with_real_arithmetic(game):
    """The eight full games at S = 128 that the GPU test plays: on every draw the numpy replay
    picks the exact index, and the draw lies 12,288 u or more inside its interval (so the
    kernel must certify it); pyoracle.mixed_playout_arena with per-seat weights plays the
    same game."""
    from oracle import pyoracle as O
    (scores, wm, plies, passes, turns), draws = H.full_game_referee(game)
    assert plies > 40 and len(draws) == plies
    for ply, (k, j, d) in enumerate(draws):
        assert k == j, (game, ply)
        assert d >= 12288 * H.ULP, (game, ply, d)
    ref = O.mixed_playout_arena(O.new_board(), H.full_game_seeds(game), 0xF,
                                weights=[H.FULL_SETS[k] for k in H.full_game_seat_sets(game)])
    assert (list(ref[0]), ref[1], ref[2], ref[3], ref[4]) == (scores, wm, plies, passes, turns)
    assert sorted(H.full_game_seat_sets(game)) == [0, 1, 2, 3]


def test_exact_cursors_and_the_ends_they_sit_on():
    """The kept cursors draw exactly 1/4, 1/2 and 7/8, and under all-zero weights those draws
    are interval ends K / n between two pieces and between two orientations of a piece."""
    assert sorted(H.EXACT_CURSORS) == [1 << 51, 1 << 52, 7 << 50] and H.WEIGHT_SETS[H.ZERO_SET] == (0.0,) * 4
    for u53, cur in H.EXACT_CURSORS.items():
        assert H.random_sample(cur)[0] == u53
    kinds = []
    for pair in H.pairs():
        n = len(pair.pos.moves)
        if pair.set_index == H.ZERO_SET and n > 1:
            for u53 in H.EXACT_CURSORS:
                if (u53 * n) % H.TWO53 == 0:
                    j = u53 * n >> 53
                    assert pair.lo[j] == H.u_decimal(u53) and H.exact_choice(pair.hi, u53) == j
                    kinds.append(pair.pos.boundary_kind(j))
    assert kinds.count("piece") >= 2 and kinds.count("orientation") >= 2
