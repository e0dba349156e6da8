"""The learned evaluator without a GPU: host_probabilities (the kernel's specification, CPython
floats) against the reference's recorded decision_function and probabilities
(tests/golden/winprob_eval.json, tools/gen_winprob_eval_fixtures.py), model loading, and the
binding with its argument checks.

Tolerances.  sklearn scales with numpy and sums with BLAS, in another order than the chain
here, so a recorded logit t is compared within the rounding bound of a 35-term sum with three
roundings per term: 64 * 2^-53 * (|intercept| + sum |u_k|), computed per pair (about 20 times
the worst difference seen, 3.1 of these units).  A probability is the mean of three sigmoids
(slope <= 1/4): a quarter of the largest of its three logit bounds, plus 4 * 2^-53 for exp,
the add, the divides and the mean."""
import ctypes
import json
import math

import numpy as np
import pytest

from reinforcementlearning_blokus_amd import _native as N
from reinforcementlearning_blokus_amd.analytics.winprob.features import SNAPSHOT_FEATURE_COLUMNS as COLUMNS
from reinforcementlearning_blokus_amd.mcts.learned_evaluator import (LearnedWinProbabilityEvaluator, WinProbModel,
                                                                     host_probabilities)
from tests.conftest import load_golden

FIX = load_golden("winprob_eval.json")
EPS = 2.0 ** -53


def logit_bounds(model, rows):
    """[4][3] rounding bounds of the pair logits of one position."""
    out = []
    for p in range(4):
        out.append([64 * EPS * (abs(model.intercept) + sum(
            abs(((rows[p][k] - rows[q][k]) - model.mean[k]) / model.scale[k] * model.coef[k]) for k in range(34)))
            for q in range(4) if q != p])
    return out


def check_against_reference(model, rows, logits, probs, want_logits, want_probs, where):
    """Computed logits / probabilities of one position against the reference's, within the
    module's bounds; returns the worst differences in units of their bounds."""
    bounds = logit_bounds(model, rows)
    worst = 0.0
    for p in range(4):
        if want_logits is not None:
            for j in range(3):
                d = abs(logits[p][j] - want_logits[p][j])
                assert d <= bounds[p][j], (where, p, j, logits[p][j], want_logits[p][j], bounds[p][j])
                worst = max(worst, d / bounds[p][j])
        tol = max(bounds[p]) / 4 + 4 * EPS
        assert abs(probs[p] - want_probs[p]) <= tol, (where, p, probs[p], want_probs[p], tol)
    return worst


def test_fixture_covers_what_the_tests_rely_on():
    assert FIX["columns"] == COLUMNS and FIX["max_turns"] == 2500 and len(FIX["positions"]) == 60
    assert all(FIX["coverage"].values())
    flat = [p for r in FIX["positions"] for p in r["prob"]]
    assert min(flat) < 0.05 and max(flat) > 0.95
    ply0 = [r for r in FIX["positions"] if r["move_count"] == 0]
    assert ply0 and len(set(ply0[0]["prob"])) == 1


def test_host_probabilities_equal_the_reference():
    model = WinProbModel.from_dict(FIX["model"])
    worst = 0.0
    for r in FIX["positions"]:
        probs, logits = host_probabilities(model, r["rows"], with_logits=True)
        assert all(type(v) is float for v in probs)
        worst = max(worst, check_against_reference(model, r["rows"], logits, probs, r["logit"], r["prob"],
                                                   (r["num_moves"], r["seed"])))
    print(f"worst logit difference: {worst:.3f} of the bound")
    ev_rows = {name: dict(zip(COLUMNS, row)) for name, row in zip(("RED", "BLUE", "YELLOW", "GREEN"),
                                                                  FIX["positions"][7]["rows"])}
    assert host_probabilities(model, ev_rows) == host_probabilities(model, FIX["positions"][7]["rows"])
    with pytest.raises(ValueError):
        host_probabilities(model, FIX["positions"][7]["rows"][:3])


def test_subset_model_maps_onto_canonical_columns():
    doc = FIX["model_subset"]
    model = WinProbModel.from_dict(doc)
    cols = doc["feature_columns"]
    assert len(cols) == 20 and cols != sorted(cols, key=COLUMNS.index) and model.feature_columns == cols
    for c in COLUMNS:
        k = COLUMNS.index(c)
        if c in cols:
            j = cols.index(c)
            assert (model.mean[k], model.scale[k], model.coef[k]) == (float(doc["mean"][j]), float(doc["scale"][j]),
                                                                      float(doc["coef"][j])), c
        else:
            assert (model.mean[k], model.scale[k], model.coef[k]) == (0.0, 1.0, 0.0), c
    for r in FIX["positions"]:
        probs, logits = host_probabilities(model, r["rows"], with_logits=True)
        check_against_reference(model, r["rows"], logits, probs, None, r["prob_subset"], (r["num_moves"], r["seed"]))


def test_dict_round_trip_is_exact(tmp_path):
    for key in ("model", "model_subset"):
        model = WinProbModel.from_dict(FIX[key])
        doc = json.loads(json.dumps(model.to_dict()))
        assert doc == FIX[key]
        again = WinProbModel.from_dict(doc)
        assert (again.mean, again.scale, again.coef, again.intercept, again.feature_columns) == \
               (model.mean, model.scale, model.coef, model.intercept, model.feature_columns)
        path = tmp_path / f"{key}.json"
        path.write_text(json.dumps(doc))
        ev = LearnedWinProbabilityEvaluator(str(path), potential_mode="logit")
        assert ev.model_type == "pairwise_logreg" and ev.feature_columns == model.feature_columns
        assert ev.max_turns == 2500 and ev.model.coef == model.coef
        r = FIX["positions"][11]
        assert ev.host_probabilities(r["rows"]) == host_probabilities(model, r["rows"])
    native = model.as_native()
    assert list(native.coef) == model.coef and list(native.scale) == model.scale and native.intercept == model.intercept


def test_very_large_logits_saturate():
    base = WinProbModel.from_dict(FIX["model"])
    big = WinProbModel(base.mean, base.scale, [c * 1e6 for c in base.coef], base.intercept)
    seen = set()
    for r in FIX["positions"]:
        for p in host_probabilities(big, r["rows"]):
            assert 0.0 <= p <= 1.0
            seen.add(p)
    assert 0.0 in seen and 1.0 in seen
    zero = WinProbModel([0.0] * 34, [1.0] * 34, [0.0] * 34, 0.0)
    assert host_probabilities(zero, FIX["positions"][3]["rows"]) == [0.5] * 4


def test_dummy_evaluator_needs_no_model_and_no_launch():
    ev = LearnedWinProbabilityEvaluator("models/dummy_model.json")
    assert ev.model_type == "dummy" and ev.feature_columns == []
    assert ev.predict_player_win_probability(None, None) == 0.5 and ev.potential(None, None) == 0.5
    assert ev.predict_many([None, None]).tolist() == [[0.5] * 4] * 2
    assert ev.host_probabilities(FIX["positions"][0]["rows"]) == [0.5] * 4


class _Est:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _fake(name, **kw):
    return type(name, (_Est,), {})(**kw)


def _pipe(*steps):
    return _Est(steps=[(type(s).__name__.lower(), s) for s in steps])


def test_unsupported_models_raise(tmp_path):
    good = dict(FIX["model_subset"])
    with pytest.raises(ValueError, match="pairwise_gbt_phase"):
        WinProbModel.from_dict(dict(good, model_type="pairwise_gbt_phase"))
    with pytest.raises(ValueError, match="not_a_feature"):
        WinProbModel.from_dict(dict(good, feature_columns=["not_a_feature"] + good["feature_columns"][1:]))
    with pytest.raises(ValueError, match="repeats"):
        WinProbModel.from_dict(dict(good, feature_columns=[good["feature_columns"][1]] + good["feature_columns"][1:]))
    with pytest.raises(ValueError, match="lacks"):
        WinProbModel.from_dict({k: v for k, v in good.items() if k != "scale"})
    with pytest.raises(ValueError, match="scale of 0"):
        WinProbModel.from_dict(dict(good, scale=["0.0"] + good["scale"][1:]))
    with pytest.raises(ValueError, match="non-finite"):
        WinProbModel.from_dict(dict(good, coef=["nan"] + good["coef"][1:]))
    cols = COLUMNS[:3]
    logreg = _fake("LogisticRegression", coef_=np.array([[0.5, -1.0, 2.0]]), intercept_=np.array([0.25]),
                   classes_=np.array([0, 1]))
    scaler = _fake("StandardScaler", with_mean=True, with_std=True, mean_=np.array([1.0, 2.0, 3.0]),
                   scale_=np.array([2.0, 4.0, 8.0]))
    m = WinProbModel.from_pipeline(_pipe(scaler, logreg), cols)
    assert (m.mean[:4], m.scale[:4], m.coef[:4], m.intercept) == ([1.0, 2.0, 3.0, 0.0], [2.0, 4.0, 8.0, 1.0],
                                                                  [0.5, -1.0, 2.0, 0.0], 0.25)
    plain = _fake("StandardScaler", with_mean=False, with_std=False, mean_=None, scale_=None)
    m = WinProbModel.from_pipeline(_pipe(plain, logreg), cols)
    assert (m.mean[:3], m.scale[:3]) == ([0.0] * 3, [1.0] * 3)
    assert WinProbModel.from_pipeline(_pipe(logreg), cols).coef[:3] == [0.5, -1.0, 2.0]
    with pytest.raises(ValueError, match="PCA"):
        WinProbModel.from_pipeline(_pipe(_fake("PCA"), logreg), cols)
    with pytest.raises(ValueError, match="steps"):
        WinProbModel.from_pipeline(_pipe(scaler, _fake("GradientBoostingClassifier")), cols)
    multi = _fake("LogisticRegression", coef_=np.zeros((3, 3)), intercept_=np.zeros(3), classes_=np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="not binary"):
        WinProbModel.from_pipeline(_pipe(scaler, multi), cols)
    with pytest.raises(ValueError, match="feature_columns"):
        WinProbModel.from_pipeline(_pipe(scaler, logreg), COLUMNS[:4])


def test_sklearn_artifact_equals_the_json_path(tmp_path):
    pytest.importorskip("sklearn")
    joblib = pytest.importorskip("joblib")
    from sklearn.ensemble import GradientBoostingClassifier
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    rng = np.random.RandomState(5)
    cols = [COLUMNS[i] for i in rng.permutation(34)[:9]]
    X = rng.normal(size=(200, 9)) * rng.uniform(0.5, 20.0, size=9)
    y = (X @ rng.normal(size=9) + rng.normal(size=200) > 0).astype(int)
    for scaler in (StandardScaler(), StandardScaler(with_mean=False), None):
        steps = ([("scaler", scaler)] if scaler is not None else []) + [("model", LogisticRegression(max_iter=500))]
        pipe = Pipeline(steps).fit(X, y)
        pkl = tmp_path / "artifact.pkl"
        joblib.dump({"model_type": "pairwise_logreg", "feature_columns": cols, "pipeline": pipe}, pkl)
        from_pkl = WinProbModel.from_artifact(str(pkl))
        js = tmp_path / "artifact.json"
        js.write_text(json.dumps(from_pkl.to_dict()))
        from_json = WinProbModel.from_artifact(str(js))
        assert (from_pkl.mean, from_pkl.scale, from_pkl.coef, from_pkl.intercept, from_pkl.feature_columns) == \
               (from_json.mean, from_json.scale, from_json.coef, from_json.intercept, cols)
        if scaler is not None and not scaler.with_mean:
            assert from_pkl.mean == [0.0] * 34
        rows = rng.normal(size=(4, 34)).tolist()
        _, logits = host_probabilities(from_pkl, rows, with_logits=True)
        x = np.array([[rows[0][COLUMNS.index(c)] - rows[1][COLUMNS.index(c)] for c in cols]])
        assert abs(logits[0][0] - float(pipe.decision_function(x)[0])) <= logit_bounds(from_pkl, rows)[0][0]
    joblib.dump({"model_type": "pairwise_gbt_phase", "feature_columns": cols, "phase_models": {}}, pkl)
    with pytest.raises(ValueError, match="pairwise_gbt_phase"):
        LearnedWinProbabilityEvaluator(str(pkl))
    gbt = Pipeline([("model", GradientBoostingClassifier(n_estimators=2))]).fit(X, y)
    joblib.dump({"model_type": "pairwise_logreg", "feature_columns": cols, "pipeline": gbt}, pkl)
    with pytest.raises(ValueError, match="GradientBoostingClassifier"):
        WinProbModel.from_artifact(str(pkl))
    three = Pipeline([("model", LogisticRegression(max_iter=200))]).fit(X, np.arange(200) % 3)
    with pytest.raises(ValueError, match="not binary"):
        WinProbModel.from_pipeline(three, cols)


def test_binding_and_argument_checks():
    lib = N.load()
    assert lib.bk_abi_version() == N.ABI_VERSION == 7
    assert lib.bk_winprob_model_size() == ctypes.sizeof(N.BkWinprobModel) == 8 * (3 * 34 + 1) == 824
    assert {"bk_winprob_eval", "bk_winprob_model_size"} <= set(N.EXPORTS)
    model = WinProbModel.from_dict(FIX["model"]).as_native()
    states = np.zeros(1, dtype=N.STATE_DTYPE)
    sets = N.fset_new(1)
    prob, logit, status = np.zeros((1, 4)), np.zeros((1, 4, 3)), np.zeros(1, np.uint8)

    def call(h=None, st=states.ctypes.data, fs=sets.ctypes.data, n=1, ti=None, max_turns=2500, model=model,
             prob=prob.ctypes.data, logit=logit.ctypes.data, status=status.ctypes.data, mem=N.MEM_HOST):
        return lib.bk_winprob_eval(h, ctypes.c_void_p(st), ctypes.c_void_p(fs), n, ti, max_turns,
                                   ctypes.byref(model) if model is not None else None, ctypes.c_void_p(prob),
                                   ctypes.c_void_p(logit), ctypes.c_void_p(status), mem)

    # every check runs before any GPU work; without a handle each of these is BK_EINVAL (a GPU
    # test repeats the model checks on a live handle and reads their messages)
    assert call() == N.EINVAL
    for bad in (dict(st=None), dict(fs=None), dict(model=None), dict(prob=None), dict(status=None), dict(n=-1),
                dict(max_turns=-1), dict(mem=2)):
        assert call(**bad) == N.EINVAL, bad
    nan = WinProbModel.from_dict(FIX["model"]).as_native()
    nan.coef[3] = math.nan
    zero = WinProbModel.from_dict(FIX["model"]).as_native()
    zero.scale[33] = 0.0
    assert call(model=nan) == N.EINVAL and call(model=zero) == N.EINVAL
    assert not prob.any() and not logit.any() and not status.any()
