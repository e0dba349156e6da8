"""Learned win-probability evaluator (reference: mcts/learned_evaluator.py).

The reference's evaluator extracts the 34 snapshot features of all four players (four move
generations and a flood fill in Python) and feeds their pairwise differences to an sklearn
pipeline.  Here the whole evaluation -- the features and the model -- is one launch for any
number of boards.  ``host_probabilities`` / ``host_probabilities_gbt`` are the same arithmetic
in CPython floats over rows that are already computed: the kernels' specification, and the
path that needs no GPU.

Both of the reference's model types are supported:

* ``pairwise_logreg`` (WinProbModel: an optional StandardScaler, then a binary
  LogisticRegression) -- bk_winprob_eval, k_winprob; the model travels as four arrays in the
  kernel arguments.
* ``pairwise_gbt_phase`` (GbtPhaseModel: one binary sklearn GradientBoostingClassifier per
  game phase early / mid / late, picked by the pair's mean board occupancy, with a fallback
  model; an optional StandardScaler in front) -- bk_winprob_eval_gbt, k_winprob_gbt; the trees
  are uploaded once per handle (bk_gbt_model_load) and found again by the model's value key.
  The raw score equals sklearn's decision_function bit for bit.  Histogram-based boosters,
  other losses, multiclass models and custom init estimators are refused at load.
"""
from __future__ import annotations

import json
import math
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np

from ..analytics.winprob.features import SNAPSHOT_FEATURE_COLUMNS
from ..engine.board import Board, Player, pack_fsets, pack_states

_N = len(SNAPSHOT_FEATURE_COLUMNS)
_COLUMN_INDEX = {c: i for i, c in enumerate(SNAPSHOT_FEATURE_COLUMNS)}


class WinProbModel:
    """A pairwise logistic regression over differences of snapshot rows: ``mean``, ``scale``
    and ``coef`` as 34 floats each in SNAPSHOT_FEATURE_COLUMNS order, and ``intercept``.
    ``feature_columns`` is the artifact's own column list (a subset or a permutation of the
    34); columns it lacks have coef 0, mean 0 and scale 1, which contribute exactly 0."""

    def __init__(self, mean: Sequence[float], scale: Sequence[float], coef: Sequence[float], intercept: float,
                 feature_columns: Optional[Sequence[str]] = None):
        self.mean = [float(v) for v in mean]
        self.scale = [float(v) for v in scale]
        self.coef = [float(v) for v in coef]
        self.intercept = float(intercept)
        self.feature_columns = list(SNAPSHOT_FEATURE_COLUMNS if feature_columns is None else feature_columns)
        if not (len(self.mean) == len(self.scale) == len(self.coef) == _N):
            raise ValueError(f"WinProbModel: mean, scale and coef need {_N} entries each")
        values = self.mean + self.scale + self.coef + [self.intercept]
        if not all(math.isfinite(v) for v in values):
            raise ValueError("WinProbModel: the model holds a non-finite value")
        if any(v == 0.0 for v in self.scale):
            raise ValueError("WinProbModel: a scale of 0")

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_columns(cls, feature_columns: Sequence[str], mean: Sequence[float], scale: Sequence[float],
                     coef: Sequence[float], intercept: float) -> "WinProbModel":
        """The model of an artifact whose arrays follow ``feature_columns``, mapped onto the
        canonical column positions."""
        columns = [str(c) for c in feature_columns]
        if not (len(columns) == len(mean) == len(scale) == len(coef)):
            raise ValueError(f"WinProbModel: {len(columns)} feature_columns for arrays of "
                             f"{len(mean)}, {len(scale)} and {len(coef)} entries")
        unknown = [c for c in columns if c not in _COLUMN_INDEX]
        if unknown:
            raise ValueError(f"WinProbModel: feature_columns outside SNAPSHOT_FEATURE_COLUMNS: {unknown}")
        if len(set(columns)) != len(columns):
            raise ValueError("WinProbModel: feature_columns repeats a column")
        full_mean, full_scale, full_coef = [0.0] * _N, [1.0] * _N, [0.0] * _N
        for c, m, s, w in zip(columns, mean, scale, coef):
            k = _COLUMN_INDEX[c]
            full_mean[k], full_scale[k], full_coef[k] = float(m), float(s), float(w)
        return cls(full_mean, full_scale, full_coef, intercept, columns)

    @classmethod
    def from_dict(cls, doc: Mapping[str, Any]) -> "WinProbModel":
        """The JSON form: ``feature_columns``, ``mean``, ``scale``, ``coef`` (one entry per
        column, numbers or their ``repr`` strings) and ``intercept``."""
        model_type = doc.get("model_type", "pairwise_logreg")
        if model_type != "pairwise_logreg":
            raise ValueError(f"Unsupported learned evaluator model_type '{model_type}' (only pairwise_logreg)")
        try:
            columns = doc["feature_columns"]
            arrays = [[float(v) for v in doc[k]] for k in ("mean", "scale", "coef")]
            intercept = float(doc["intercept"])
        except KeyError as e:
            raise ValueError(f"WinProbModel: the model document lacks {e.args[0]!r}") from None
        return cls.from_columns(columns, arrays[0], arrays[1], arrays[2], intercept)

    def to_dict(self) -> Dict[str, Any]:
        """Plain JSON; doubles as ``repr`` strings, which round-trip exactly."""
        idx = [_COLUMN_INDEX[c] for c in self.feature_columns]
        return {"model_type": "pairwise_logreg", "feature_columns": list(self.feature_columns),
                "mean": [repr(self.mean[k]) for k in idx], "scale": [repr(self.scale[k]) for k in idx],
                "coef": [repr(self.coef[k]) for k in idx], "intercept": repr(self.intercept)}

    @classmethod
    def from_pipeline(cls, pipeline, feature_columns: Sequence[str]) -> "WinProbModel":
        """An sklearn Pipeline: an optional StandardScaler, then a binary LogisticRegression."""
        steps = [est for _, est in getattr(pipeline, "steps", [("model", pipeline)])]
        kinds = [type(est).__name__ for est in steps]
        if not steps or kinds[-1] != "LogisticRegression" or kinds[:-1] not in ([], ["StandardScaler"]):
            raise ValueError(f"WinProbModel: unsupported pipeline steps {kinds} "
                             "(an optional StandardScaler, then LogisticRegression)")
        logreg = steps[-1]
        coef = np.asarray(logreg.coef_, dtype=np.float64)
        if coef.ndim != 2 or coef.shape[0] != 1 or len(getattr(logreg, "classes_", [0, 1])) != 2:
            raise ValueError("WinProbModel: the LogisticRegression is not binary")
        n = coef.shape[1]
        mean, scale = np.zeros(n), np.ones(n)
        if len(steps) == 2:
            scaler = steps[0]
            if getattr(scaler, "with_mean", True) and getattr(scaler, "mean_", None) is not None:
                mean = np.asarray(scaler.mean_, dtype=np.float64)
            if getattr(scaler, "with_std", True) and getattr(scaler, "scale_", None) is not None:
                scale = np.asarray(scaler.scale_, dtype=np.float64)
        intercept = float(np.asarray(logreg.intercept_, dtype=np.float64).reshape(-1)[0])
        return cls.from_columns(feature_columns, mean.tolist(), scale.tolist(), coef[0].tolist(), intercept)

    @classmethod
    def from_artifact(cls, path: str) -> "WinProbModel":
        """The reference's joblib artifact ``{"model_type": "pairwise_logreg", "feature_columns":
        [...], "pipeline": Pipeline}``, or this package's ``.json`` form (no pickle involved)."""
        path = str(path)
        if path.endswith(".json"):
            with open(path) as fh:
                return cls.from_dict(json.load(fh))
        import joblib  # only for the reference's pickled artifacts
        artifact = joblib.load(path)
        model_type = str(artifact.get("model_type", ""))
        if model_type != "pairwise_logreg":
            raise ValueError(f"Unsupported learned evaluator model_type '{model_type}' in {path} "
                             "(only pairwise_logreg)")
        return cls.from_pipeline(artifact["pipeline"], artifact.get("feature_columns", SNAPSHOT_FEATURE_COLUMNS))

    # ------------------------------------------------------------------ use
    def as_native(self):
        """The bk_winprob_model (cached: the arrays are not meant to change)."""
        native = self.__dict__.get("_native")
        if native is None:
            from .. import _native as N
            native = N.BkWinprobModel()
            for k in range(_N):
                native.mean[k], native.scale[k], native.coef[k] = self.mean[k], self.scale[k], self.coef[k]
            native.intercept = self.intercept
            self.__dict__["_native"] = native
        return native

    def key(self):
        """The model's values as one hashable (cached): equal keys, the same arithmetic."""
        k = self.__dict__.get("_key")
        if k is None:
            k = self.__dict__["_key"] = (tuple(self.mean), tuple(self.scale), tuple(self.coef), self.intercept)
        return k

    def pair_logit(self, row_p: Sequence[float], row_q: Sequence[float]) -> float:
        """t of player p against q: the kernel's chain, one rounding per operation."""
        t = 0.0
        for k in range(_N):
            t = t + ((row_p[k] - row_q[k]) - self.mean[k]) / self.scale[k] * self.coef[k]
        return t + self.intercept


def _sigmoid(t: float) -> float:
    try:
        e = math.exp(-t)
    except OverflowError:  # C's exp returns +inf here, as the kernel's does
        e = math.inf
    return 1.0 / (1.0 + e)


def _rows(rows) -> List[List[float]]:
    if isinstance(rows, Mapping):  # {Player.name or player: feature dict}, as snapshot_features_many gives
        rows = list(rows.values())
    out = [[float(r[c]) for c in SNAPSHOT_FEATURE_COLUMNS] if isinstance(r, Mapping) else [float(v) for v in r]
           for r in rows]
    if len(out) != 4 or any(len(r) != _N for r in out):
        raise ValueError(f"host_probabilities: four rows of {_N} features are needed")
    return out


def host_probabilities(model: WinProbModel, rows, *, with_logits: bool = False):
    """The four players' win probabilities from their feature rows ([4][34] in
    SNAPSHOT_FEATURE_COLUMNS order, players in id order) in CPython floats: for player p and
    each opponent q in ascending id, x_k = f[p][k] - f[q][k], z_k = (x_k - mean_k) / scale_k,
    u_k = z_k * coef_k, t = ((..(0 + u_0) + ..) + u_33) + intercept, s = 1 / (1 + exp(-t));
    the probability is ((s_0 + s_1) + s_2) / 3.0.  With ``with_logits`` also the 4 x 3 t."""
    f = _rows(rows)
    probs, logits = [], []
    for p in range(4):
        ts = [model.pair_logit(f[p], f[q]) for q in range(4) if q != p]
        s = [_sigmoid(t) for t in ts]
        probs.append(((s[0] + s[1]) + s[2]) / 3.0)
        logits.append(ts)
    return (probs, logits) if with_logits else probs


GBT_PHASES = ("early", "mid", "late")
_OCC = _COLUMN_INDEX["phase_board_occupancy"]
GBT_TYPE = "pairwise_gbt_phase"


def gbt_phase(occupancy: float) -> int:
    """The reference's _phase_bucket_from_occupancy as an index into GBT_PHASES."""
    return 0 if occupancy < 0.33 else (1 if occupancy < 0.66 else 2)


class GbtEnsemble:
    """One binary GradientBoostingClassifier: ``init`` (the raw prior), ``learning_rate`` and
    the stages' trees in one node array.  ``roots[s]`` is stage s's root; node i is a leaf with
    value ``tv[i]`` when ``left[i] == -1``, else it sends a row left (to ``left[i]``) when
    ``float32(row)[feature[i]] <= tv[i]`` and right (to ``left[i] + 1``) otherwise.  Children
    have larger indices than their parent.  ``feature`` holds canonical column positions."""

    def __init__(self, init: float, learning_rate: float, roots: Sequence[int], left: Sequence[int],
                 feature: Sequence[int], tv: Sequence[float]):
        self.init, self.learning_rate = float(init), float(learning_rate)
        self.roots = [int(v) for v in roots]
        self.left, self.feature = [int(v) for v in left], [int(v) for v in feature]
        self.tv = [float(v) for v in tv]
        n = len(self.tv)
        if not (len(self.left) == len(self.feature) == n) or n < 1:
            raise ValueError(f"{GBT_TYPE}: left, feature and tv need one entry per node, and a node")
        if not self.roots:
            raise ValueError(f"{GBT_TYPE}: an ensemble without a stage")
        if not all(math.isfinite(v) for v in self.tv + [self.init, self.learning_rate]):
            raise ValueError(f"{GBT_TYPE}: the ensemble holds a non-finite value")
        if any(not 0 <= r < n for r in self.roots):
            raise ValueError(f"{GBT_TYPE}: a tree root outside the {n} nodes")
        for i, (lf, f) in enumerate(zip(self.left, self.feature)):
            if not 0 <= f < _N:
                raise ValueError(f"{GBT_TYPE}: node {i} tests feature {f}, outside 0..{_N - 1}")
            if lf != -1 and not i < lf < n - 1:
                raise ValueError(f"{GBT_TYPE}: node {i} has children {lf} and {lf + 1}; they must follow it "
                                 f"inside the {n} nodes")

    def key(self):
        return (self.init, self.learning_rate, tuple(self.roots), tuple(self.left), tuple(self.feature),
                tuple(self.tv))

    def raw(self, xf: Sequence[float]) -> float:
        """decision_function of one float32 row (as floats): init, then + learning_rate * leaf
        stage by stage, one rounding per operation."""
        t = self.init
        left, feature, tv = self.left, self.feature, self.tv
        for i in self.roots:
            while left[i] != -1:
                i = left[i] + (0 if xf[feature[i]] <= tv[i] else 1)
            t = t + self.learning_rate * tv[i]
        return t

    @classmethod
    def from_estimator(cls, est, positions: Sequence[int], where: str) -> "GbtEnsemble":
        """A fitted sklearn GradientBoostingClassifier whose input column c is canonical column
        ``positions[c]``."""
        kind = type(est).__name__
        if kind != "GradientBoostingClassifier":
            raise ValueError(f"{GBT_TYPE}: {where} is a {kind}; only sklearn's GradientBoostingClassifier "
                             "(optionally after a StandardScaler) is supported")
        loss = getattr(est, "loss", None)
        if loss not in ("log_loss", "deviance"):
            raise ValueError(f"{GBT_TYPE}: {where} was fitted with loss {loss!r}; only log_loss is supported")
        stages = np.asarray(est.estimators_, dtype=object)
        if len(getattr(est, "classes_", [0, 1])) != 2 or stages.ndim != 2 or stages.shape[1] != 1:
            raise ValueError(f"{GBT_TYPE}: {where} is a multiclass model; only binary models are supported")
        if int(getattr(est, "n_features_in_", len(positions))) != len(positions):
            raise ValueError(f"{GBT_TYPE}: {where} takes {est.n_features_in_} features, the artifact has "
                             f"{len(positions)} feature_columns")
        if isinstance(est.init, str) and est.init == "zero":
            init = 0.0
        elif est.init is None:  # the prior's raw score, as the fitted model adds it
            prior = est._raw_predict_init(np.zeros((1, len(positions))))
            init = float(np.asarray(prior, dtype=np.float64).reshape(-1)[0])
        else:
            raise ValueError(f"{GBT_TYPE}: {where} has a custom init estimator ({type(est.init).__name__}); only "
                             "the default prior and init='zero' are supported")
        roots, left, feature, tv = [], [], [], []
        for stage in stages[:, 0]:
            tree = stage.tree_
            cl, cr = tree.children_left, tree.children_right
            order = [0]  # breadth first: a node's children are adjacent and follow it
            base = len(tv)
            roots.append(base)
            at = 0
            while at < len(order):
                i = order[at]
                at += 1
                if cl[i] == -1:
                    left.append(-1)
                    feature.append(0)
                    tv.append(float(tree.value[i, 0, 0]))
                else:
                    left.append(base + len(order))
                    feature.append(positions[int(tree.feature[i])])
                    tv.append(float(tree.threshold[i]))
                    order += [int(cl[i]), int(cr[i])]
        return cls(init, float(est.learning_rate), roots, left, feature, tv)


def _scaler_arrays(scaler, n: int, where: str):
    kind = type(scaler).__name__
    if kind != "StandardScaler":
        raise ValueError(f"{GBT_TYPE}: {where} starts with a {kind}; only a StandardScaler may precede the classifier")
    mean, scale = np.zeros(n), np.ones(n)
    if getattr(scaler, "with_mean", True) and getattr(scaler, "mean_", None) is not None:
        mean = np.asarray(scaler.mean_, dtype=np.float64)
    if getattr(scaler, "with_std", True) and getattr(scaler, "scale_", None) is not None:
        scale = np.asarray(scaler.scale_, dtype=np.float64)
    if len(mean) != n or len(scale) != n:
        raise ValueError(f"{GBT_TYPE}: {where}'s StandardScaler has {len(mean)} columns, the artifact {n}")
    return mean.tolist(), scale.tolist()


class GbtPhaseModel:
    """The reference's ``pairwise_gbt_phase`` evaluator: one GbtEnsemble per game phase over
    differences of snapshot rows, behind an optional StandardScaler (``mean`` and ``scale``, 34
    floats each in SNAPSHOT_FEATURE_COLUMNS order; 0 and 1 where absent).  ``ensembles`` are
    the distinct ensembles and ``phase_ensemble[ph]`` the one of GBT_PHASES[ph]: the phases
    are resolved here, once, as the reference resolves them per call (``phase_models.get(phase)
    or fallback_model``), and a phase that resolves to nothing is an error at load.  One scaler
    serves every ensemble (bk_gbt_model holds one): pipelines that disagree are refused."""

    def __init__(self, ensembles: Sequence[GbtEnsemble], phase_ensemble: Sequence[int],
                 mean: Optional[Sequence[float]] = None, scale: Optional[Sequence[float]] = None,
                 feature_columns: Optional[Sequence[str]] = None):
        self.ensembles = list(ensembles)
        self.phase_ensemble = [int(v) for v in phase_ensemble]
        self.mean = [0.0] * _N if mean is None else [float(v) for v in mean]
        self.scale = [1.0] * _N if scale is None else [float(v) for v in scale]
        self.feature_columns = list(SNAPSHOT_FEATURE_COLUMNS if feature_columns is None else feature_columns)
        if len(self.phase_ensemble) != 3 or any(not 0 <= e < len(self.ensembles) for e in self.phase_ensemble):
            raise ValueError(f"{GBT_TYPE}: phase_ensemble needs one ensemble index per phase {GBT_PHASES}")
        if not (len(self.mean) == len(self.scale) == _N):
            raise ValueError(f"{GBT_TYPE}: mean and scale need {_N} entries each")
        if not all(math.isfinite(v) for v in self.mean + self.scale):
            raise ValueError(f"{GBT_TYPE}: the scaler holds a non-finite value")
        if any(v == 0.0 for v in self.scale):
            raise ValueError(f"{GBT_TYPE}: a scale of 0")

    # ------------------------------------------------------------------ construction
    @staticmethod
    def _positions(feature_columns: Sequence[str]) -> List[int]:
        columns = [str(c) for c in feature_columns]
        unknown = [c for c in columns if c not in _COLUMN_INDEX]
        if unknown:
            raise ValueError(f"{GBT_TYPE}: feature_columns outside SNAPSHOT_FEATURE_COLUMNS: {unknown}")
        if len(set(columns)) != len(columns):
            raise ValueError(f"{GBT_TYPE}: feature_columns repeats a column")
        return [_COLUMN_INDEX[c] for c in columns]

    @classmethod
    def _resolve(cls, named: Mapping[str, Any], fallback, what: str, same=lambda a, b: a is b):
        """(distinct models, [index per phase]) of ``phase_models.get(phase) or fallback_model``."""
        if not any(named.get(ph) is not None for ph in GBT_PHASES) and fallback is None:
            raise ValueError(f"{GBT_TYPE}: {what} has neither phase models nor a fallback_model")
        models, index = [], []
        for ph in GBT_PHASES:
            m = named.get(ph)
            m = fallback if m is None else m
            if m is None:
                raise ValueError(f"{GBT_TYPE}: {what} has no model for phase '{ph}' and no fallback_model")
            at = next((i for i, have in enumerate(models) if same(have, m)), None)
            if at is None:
                at = len(models)
                models.append(m)
            index.append(at)
        return models, index

    @classmethod
    def from_models(cls, phase_models: Mapping[str, Any], fallback_model,
                    feature_columns: Sequence[str]) -> "GbtPhaseModel":
        """sklearn models as the reference's artifact holds them: each a binary
        GradientBoostingClassifier, bare or as the last step of a Pipeline after an optional
        StandardScaler."""
        positions = cls._positions(feature_columns)
        models, index = cls._resolve(dict(phase_models or {}), fallback_model, "the artifact")
        ensembles, scalers = [], []
        for i, m in enumerate(models):
            where = "the " + " / ".join(GBT_PHASES[p] for p in range(3) if index[p] == i) + " model"
            steps = [est for _, est in getattr(m, "steps", [("model", m)])]
            if len(steps) > 2 or not steps:
                raise ValueError(f"{GBT_TYPE}: {where} is a pipeline of {[type(s).__name__ for s in steps]}; only an "
                                 "optional StandardScaler then a GradientBoostingClassifier is supported")
            scalers.append(_scaler_arrays(steps[0], len(positions), where) if len(steps) == 2
                           else ([0.0] * len(positions), [1.0] * len(positions)))
            ensembles.append(GbtEnsemble.from_estimator(steps[-1], positions, where))
        if any(s != scalers[0] for s in scalers):
            raise ValueError(f"{GBT_TYPE}: the phase models' StandardScalers differ; one scaler must serve every phase")
        mean, scale = [0.0] * _N, [1.0] * _N
        for k, m, s in zip(positions, *scalers[0]):
            mean[k], scale[k] = float(m), float(s)
        return cls(ensembles, index, mean, scale, [str(c) for c in feature_columns])

    @classmethod
    def from_dict(cls, doc: Mapping[str, Any]) -> "GbtPhaseModel":
        """The JSON form: ``feature_columns``; optional ``mean`` and ``scale`` (one entry per
        column); ``ensembles``, each ``{"init", "learning_rate", "roots", "left", "feature",
        "tv"}`` with ``feature`` indexing feature_columns; ``phase_models`` {phase: ensemble
        index} and ``fallback_model`` (an index or null).  Numbers or their ``repr`` strings."""
        if doc.get("model_type") != GBT_TYPE:
            raise ValueError(f"{GBT_TYPE}: the model document has model_type {doc.get('model_type')!r}")
        try:
            columns = doc["feature_columns"]
            positions = cls._positions(columns)
            raw = doc["ensembles"]
            named, fallback = doc["phase_models"], doc.get("fallback_model")
            ensembles = []
            for e in raw:
                feats = [int(f) for f in e["feature"]]
                if any(not 0 <= f < len(positions) for f in feats):
                    raise ValueError(f"{GBT_TYPE}: a node tests a feature outside the {len(positions)} feature_columns")
                ensembles.append(GbtEnsemble(float(e["init"]), float(e["learning_rate"]), e["roots"], e["left"],
                                             [positions[f] for f in feats], [float(v) for v in e["tv"]]))
        except KeyError as e:
            raise ValueError(f"{GBT_TYPE}: the model document lacks {e.args[0]!r}") from None
        for v in list(named.values()) + [fallback]:
            if v is not None and not 0 <= int(v) < len(ensembles):
                raise ValueError(f"{GBT_TYPE}: the model document names ensemble {v}, it has {len(ensembles)}")
        order, index = cls._resolve({k: (None if v is None else int(v)) for k, v in named.items()},
                                    None if fallback is None else int(fallback), "the model document",
                                    same=lambda a, b: a == b)
        mean, scale = [0.0] * _N, [1.0] * _N
        for name, full in (("mean", mean), ("scale", scale)):
            if doc.get(name) is not None:
                if len(doc[name]) != len(positions):
                    raise ValueError(f"{GBT_TYPE}: {name} has {len(doc[name])} entries for {len(positions)} "
                                     "feature_columns")
                for k, v in zip(positions, doc[name]):
                    full[k] = float(v)
        return cls([ensembles[i] for i in order], index, mean, scale, [str(c) for c in columns])

    def to_dict(self) -> Dict[str, Any]:
        """Plain JSON; doubles as ``repr`` strings, which round-trip exactly.  Every phase is
        named (the fallback is already resolved), so ``fallback_model`` is null."""
        idx = [_COLUMN_INDEX[c] for c in self.feature_columns]
        local = {k: i for i, k in enumerate(idx)}
        return {"model_type": GBT_TYPE, "feature_columns": list(self.feature_columns),
                "mean": [repr(self.mean[k]) for k in idx], "scale": [repr(self.scale[k]) for k in idx],
                "ensembles": [{"init": repr(e.init), "learning_rate": repr(e.learning_rate), "roots": list(e.roots),
                               "left": list(e.left), "feature": [local.get(f, 0) for f in e.feature],
                               "tv": [repr(v) for v in e.tv]} for e in self.ensembles],
                "phase_models": {ph: self.phase_ensemble[i] for i, ph in enumerate(GBT_PHASES)},
                "fallback_model": None}

    @classmethod
    def from_artifact(cls, path: str) -> "GbtPhaseModel":
        """The reference's joblib artifact ``{"model_type": "pairwise_gbt_phase", "feature_columns",
        "phase_models": {phase: model}, "fallback_model": model}``, or this package's ``.json``
        form (no pickle and no sklearn involved)."""
        path = str(path)
        if path.endswith(".json"):
            with open(path) as fh:
                return cls.from_dict(json.load(fh))
        import joblib  # only for the reference's pickled artifacts
        artifact = joblib.load(path)
        if str(artifact.get("model_type", "")) != GBT_TYPE:
            raise ValueError(f"{GBT_TYPE}: {path} has model_type {artifact.get('model_type')!r}")
        return cls.from_models(artifact.get("phase_models", {}), artifact.get("fallback_model"),
                               artifact.get("feature_columns", SNAPSHOT_FEATURE_COLUMNS))

    # ------------------------------------------------------------------ use
    def ensemble(self, phase: int) -> GbtEnsemble:
        return self.ensembles[self.phase_ensemble[phase]]

    def as_native(self):
        """(bk_gbt_model, tree roots int32, nodes N.GBT_NODE_DTYPE) as bk_gbt_model_load takes
        them (cached): the distinct ensembles' nodes one after the other."""
        native = self.__dict__.get("_native")
        if native is None:
            from .. import _native as N
            model = N.BkGbtModel()
            for k in range(_N):
                model.mean[k], model.scale[k] = self.mean[k], self.scale[k]
            roots, first, node_base = [], [], 0
            nodes = np.zeros(sum(len(e.tv) for e in self.ensembles), dtype=N.GBT_NODE_DTYPE)
            for e in self.ensembles:
                first.append(len(roots))
                roots += [node_base + r for r in e.roots]
                part = nodes[node_base:node_base + len(e.tv)]
                part["tv"], part["feature"] = e.tv, e.feature
                part["left"] = [-1 if lf == -1 else node_base + lf for lf in e.left]
                node_base += len(e.tv)
            for ph in range(3):
                e = self.ensemble(ph)
                model.phase[ph].init, model.phase[ph].learning_rate = e.init, e.learning_rate
                model.phase[ph].first_tree, model.phase[ph].n_trees = first[self.phase_ensemble[ph]], len(e.roots)
            native = self.__dict__["_native"] = (model, np.array(roots, dtype=np.int32), nodes)
        return native

    def key(self):
        """The model's values as one hashable (cached): equal keys, the same arithmetic."""
        k = self.__dict__.get("_key")
        if k is None:
            k = self.__dict__["_key"] = (GBT_TYPE, tuple(self.mean), tuple(self.scale), tuple(self.phase_ensemble),
                                         tuple(e.key() for e in self.ensembles))
        return k

    def pair_raw(self, row_p: Sequence[float], row_q: Sequence[float]) -> float:
        """t of player p against q: the kernel's chain."""
        with np.errstate(over="ignore"):
            xf = [float(np.float32(((row_p[k] - row_q[k]) - self.mean[k]) / self.scale[k])) for k in range(_N)]
        return self.ensemble(gbt_phase((row_p[_OCC] + row_q[_OCC]) / 2.0)).raw(xf)


def host_probabilities_gbt(model: GbtPhaseModel, rows, with_raw: bool = False):
    """host_probabilities for a GbtPhaseModel, the specification of k_winprob_gbt in CPython
    floats: for player p and each opponent q in ascending id, x_k = f[p][k] - f[q][k],
    z_k = (x_k - mean_k) / scale_k, xf_k = float32(z_k); occupancy = (f[p][occ] + f[q][occ]) /
    2.0 from the canonical phase_board_occupancy column, phase early if occupancy < 0.33, mid if
    < 0.66, else late; t = init, then t = t + learning_rate * leaf for that phase's stages in
    order, a row going left at a node when double(xf[feature]) <= threshold; s = 1 / (1 +
    exp(-t)); the probability is ((s_0 + s_1) + s_2) / 3.0.  With ``with_raw`` also the 4 x 3 t
    (sklearn's decision_function of each pair).  sklearn's missing-value branch is not
    modelled: the rows are finite."""
    f = _rows(rows)
    probs, raws = [], []
    for p in range(4):
        ts = [model.pair_raw(f[p], f[q]) for q in range(4) if q != p]
        s = [_sigmoid(t) for t in ts]
        probs.append(((s[0] + s[1]) + s[2]) / 3.0)
        raws.append(ts)
    return (probs, raws) if with_raw else probs


def _artifact_model_type(path: str) -> str:
    """The model_type an artifact declares (its loader is picked by it)."""
    if path.endswith(".json"):
        with open(path) as fh:
            doc = json.load(fh)
        return str(doc.get("model_type", "pairwise_logreg"))
    import joblib
    return str(joblib.load(path).get("model_type", ""))


class LearnedWinProbabilityEvaluator:
    """Model-backed evaluator that estimates per-player win probability (the reference's
    surface, plus ``predict_many`` and ``host_probabilities``), for both of the reference's
    model types: ``model`` is a WinProbModel or a GbtPhaseModel."""

    def __init__(self, artifact_path: str, *, max_turns: int = 2500, potential_mode: str = "prob", device: int = 0):
        self.artifact_path = str(artifact_path)
        self.max_turns = int(max_turns)
        self.potential_mode = potential_mode
        self.device = device
        self.model = None  # a WinProbModel or a GbtPhaseModel
        self._is_dummy = self.artifact_path.endswith("dummy_model.json")
        if self._is_dummy:
            self.model_type = "dummy"
            self.feature_columns: List[str] = []
            return
        if _artifact_model_type(self.artifact_path) == GBT_TYPE:
            self.model = GbtPhaseModel.from_artifact(self.artifact_path)
            self.model_type = GBT_TYPE
        else:
            self.model = WinProbModel.from_artifact(self.artifact_path)
            self.model_type = "pairwise_logreg"
        self.feature_columns = list(self.model.feature_columns)

    def _engine(self):
        from ..gpu import BlokusGPU
        return BlokusGPU.shared(self.device)

    def predict_many(self, boards: Sequence[Board]) -> np.ndarray:
        """float64 [n, 4]: every player's win probability on every board, one launch, with
        the evaluator's own context (turn_index = each board's move_count)."""
        boards = list(boards)
        if self._is_dummy or not boards:
            return np.full((len(boards), 4), 0.5)
        gbt = self.model_type == GBT_TYPE
        launch = self._engine().winprob_eval_gbt if gbt else self._engine().winprob_eval
        prob, _, status = launch(pack_states(boards), pack_fsets(boards), None, self.max_turns, self.model)
        if status.any():
            bad = int(np.flatnonzero(status)[0])
            raise RuntimeError(f"{'bk_winprob_eval_gbt' if gbt else 'bk_winprob_eval'}: board {bad} or its frontier "
                               f"tables are invalid (status {int(status[bad])})")
        return prob

    def host_probabilities(self, rows) -> List[float]:
        """The four probabilities from four feature rows that are already computed (no GPU)."""
        if self._is_dummy:
            return [0.5] * 4
        if self.model_type == GBT_TYPE:
            return host_probabilities_gbt(self.model, rows)
        return host_probabilities(self.model, rows)

    def predict_player_win_probability(self, board: Board, player: Player) -> float:
        """Estimate a player's win chance by aggregating pairwise probabilities."""
        if self._is_dummy:
            return 0.5
        return float(self.predict_many([board])[0, player.value - 1])

    def potential(self, board: Board, player: Player) -> float:
        """Potential function used for reward shaping."""
        probability = self.predict_player_win_probability(board, player)
        probability = min(max(probability, 1e-6), 1 - 1e-6)
        if self.potential_mode == "logit":
            return float(math.log(probability / (1.0 - probability)))
        return float(probability)
