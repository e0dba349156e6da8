"""What the two pairwise_gbt_phase test modules share: tests/golden/winprob_gbt.json
(tools/gen_winprob_gbt_fixtures.py) joined with the positions of winprob_eval.json it names, and
hand-built models."""
import base64
import zlib

import numpy as np

from reinforcementlearning_blokus_amd import _native as N
from reinforcementlearning_blokus_amd.mcts.learned_evaluator import GbtEnsemble, GbtPhaseModel
from tests.conftest import load_golden

FIX = load_golden("winprob_gbt.json")
EVAL = load_golden("winprob_eval.json")
ARTIFACTS = ("phases", "mid_fallback", "subset_scaled")
MAX_TURNS = FIX["max_turns"]
OCC = FIX["columns"].index("phase_board_occupancy")


def models():
    return {name: GbtPhaseModel.from_dict(FIX["models"][name]) for name in ARTIFACTS}


def positions():
    """Every fixture position with its own or winprob_eval.json's rows, state and tables."""
    out = []
    for r in FIX["positions"]:
        src = r if "state" in r else EVAL["positions"][r["eval_index"]]
        out.append(dict(r, rows=src["rows"], state=src["state"], sets=src["sets"], move_count=src["move_count"]))
    return out


def decode(text, dtype):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype=dtype).copy()


def packed(pos):
    return (np.concatenate([decode(r["state"], N.STATE_DTYPE) for r in pos]),
            np.concatenate([decode(r["sets"], N.FSET_DTYPE) for r in pos]))


def tree(spec, nodes):
    """Append the tree `spec` to `nodes` ([left, feature, tv] lists), breadth first, and return
    its root.  spec: a float (a leaf) or (feature, threshold, left spec, right spec)."""
    root = len(nodes)
    nodes.append(None)
    queue = [(root, spec)]
    while queue:
        at, s = queue.pop(0)
        if isinstance(s, tuple):
            f, thr, lo, hi = s
            nodes[at] = [len(nodes), f, float(thr)]
            queue += [(len(nodes), lo), (len(nodes) + 1, hi)]
            nodes += [None, None]
        else:
            nodes[at] = [-1, 0, float(s)]
    return root


def ensemble(specs, init=0.0, learning_rate=1.0):
    nodes, roots = [], []
    for s in specs:
        roots.append(tree(s, nodes))
    return GbtEnsemble(init, learning_rate, roots, [n[0] for n in nodes], [n[1] for n in nodes], [n[2] for n in nodes])


def one_ensemble_model(specs, init=0.0, learning_rate=1.0, mean=None, scale=None):
    return GbtPhaseModel([ensemble(specs, init, learning_rate)], [0, 0, 0], mean, scale)


def random_spec(rng, depth, span):
    """A random tree: thresholds drawn per feature from `span` ([34] typical |difference|)."""
    if depth == 0 or rng.random_sample() < 0.15:
        return float(rng.normal())
    f = int(rng.randint(34))
    return (f, float(rng.normal() * span[f]), random_spec(rng, depth - 1, span), random_spec(rng, depth - 1, span))


def synthetic_model(stages, seed, span, depth=3, leaf_scale=1.0):
    """Three different ensembles (early, mid, late) of `stages` random trees each."""
    rng = np.random.RandomState(seed)

    def scaled(s):
        return (s[0], s[1], scaled(s[2]), scaled(s[3])) if isinstance(s, tuple) else s * leaf_scale
    ens = [ensemble([scaled(random_spec(rng, depth, span)) for _ in range(stages)], float(rng.normal()), 0.1 + 0.05 * e)
           for e in range(3)]
    return GbtPhaseModel(ens, [0, 1, 2])


def chain_spec(rng, depth, span):
    """An unbalanced tree: one path of `depth` inner nodes, a leaf hanging off each; the
    thresholds lean towards the path, so some rows follow it to the end.  Returns the spec and
    the value of the deepest leaf."""
    deepest = float(rng.normal())
    spec = deepest
    for _ in range(depth):
        f = int(rng.randint(34))
        leaf, lean = float(rng.normal()), float(rng.random_sample() * span[f])
        spec = (f, -lean, leaf, spec) if rng.random_sample() < 0.5 else (f, lean, spec, leaf)
    return spec, deepest


def feature_span(pos):
    """[34] the largest |f[p][k] - f[q][k]| over the fixture positions (at least 1)."""
    span = np.ones(34)
    for r in pos:
        a = np.array(r["rows"])
        span = np.maximum(span, np.abs(a[:, None, :] - a[None, :, :]).max(axis=(0, 1)))
    return span
