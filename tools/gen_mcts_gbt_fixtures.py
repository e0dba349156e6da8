#!/usr/bin/env python3
"""Generate tests/golden/mcts_gbt.json from the reference implementation: its MCTSAgent
searching with the ``phases`` pairwise_gbt_phase artifact of tests/golden/winprob_gbt.json.

Like tools/gen_winprob_gbt_fixtures.py this imports a read-only checkout of the reference
($BLOKUS_REFERENCE) and records its behaviour; only the JSON it writes is committed.  CPU
only; needs scikit-learn and joblib, and the in-tree library built::

    cd /tmp && BLOKUS_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python <repo>/tools/gen_mcts_gbt_fixtures.py

1. The ``phases`` artifact is fitted again with the routines and random_state of
   tools/gen_winprob_gbt_fixtures.py.  The fit has to reproduce the committed model: the
   GbtPhaseModel of the new fit must have the key() of winprob_gbt.json's, or nothing is
   written (another scikit-learn may grow other trees).
2. The artifact goes to a temporary directory as the reference's joblib file, and the
   reference's MCTSAgent searches from the search position of winprob_eval.json with it: leaf
   evaluation, and leaf evaluation with progressive bias, 24 iterations each, the seeds of
   tools/gen_winprob_eval_fixtures.py.
3. Only results are recorded: the move, the counters, the root's children and the rewards.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_winprob_eval_fixtures as E  # noqa: E402  (gen_search, SEARCHES, the seeds)
import gen_winprob_gbt_fixtures as T  # noqa: E402  (fit_models, PHASES)

REF, REPO, GOLDEN = T.REF, T.REPO, T.GOLDEN
OUT = os.path.join(GOLDEN, "mcts_gbt.json")


def main():
    if not os.path.isdir(os.path.join(REF, "engine")):
        sys.exit("set BLOKUS_REFERENCE to a checkout of the reference")
    import joblib
    sys.path.insert(0, REPO)
    from reinforcementlearning_blokus_amd.analytics.winprob.features import SNAPSHOT_FEATURE_COLUMNS as COLUMNS
    from reinforcementlearning_blokus_amd.mcts.learned_evaluator import GbtPhaseModel
    COLUMNS = list(COLUMNS)
    gbt_doc = json.load(open(os.path.join(GOLDEN, "winprob_gbt.json")))
    eval_doc = json.load(open(os.path.join(GOLDEN, "winprob_eval.json")))
    assert gbt_doc["columns"] == COLUMNS and gbt_doc["random_state"] == T.RANDOM_STATE
    full, train = T.fit_models(COLUMNS, scaled=False)
    artifact = {"feature_columns": COLUMNS, "phase_models": {k: full[k] for k in T.PHASES}, "fallback_model": full["all"]}
    refit = GbtPhaseModel.from_models(artifact["phase_models"], artifact["fallback_model"], COLUMNS)
    want = GbtPhaseModel.from_dict(gbt_doc["models"]["phases"])
    if refit.key() != want.key():
        sys.exit("the fit does not reproduce winprob_gbt.json's `phases` model on this scikit-learn: nothing written")
    print(f"fitted on {train} pairs: the committed model, value for value")
    search = eval_doc["search"]
    spec = (search["num_moves"], search["seed"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "phases.pkl")
        joblib.dump(dict(artifact, model_type="pairwise_gbt_phase"), path)
        searches = [E.gen_search((spec, search["player"], path, s)) for s in E.SEARCHES[:2]]
    for s, logreg in zip(searches, search["searches"]):
        assert s["name"] == logreg["name"] and s["n_legal"] == logreg["n_legal"] and not s.pop("potential_shaping_terms")
    assert searches[0]["leaf_eval_calls"] > 0 and searches[1]["progressive_bias_updates"] > 0
    assert any(ch[2] != 0.0 for ch in searches[1]["root_children"])
    doc = {"model": "phases", "position": "winprob_eval.json search", "player": search["player"], "searches": searches}
    text = json.dumps(doc, separators=(",", ":"))
    assert len(text) < 16384, len(text)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(f"wrote {OUT}: {len(text)} bytes, reference seconds {[s['reference_seconds'] for s in searches]}")


if __name__ == "__main__":
    main()
