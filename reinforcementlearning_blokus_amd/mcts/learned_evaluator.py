"""Learned win-probability evaluator (reference: mcts/learned_evaluator.py).

The reference's evaluator extracts the 34 snapshot features of all four players (four move
generations and a flood fill in Python) and feeds their pairwise differences to an sklearn
pipeline.  Here the whole evaluation -- the features and the pairwise logistic regression --
is one bk_winprob_eval launch (k_winprob) for any number of boards; the model travels as four
arrays in the kernel arguments.  ``host_probabilities`` is the same arithmetic in CPython
floats over rows that are already computed: the kernel's specification, and the path that
needs no GPU.

Only ``pairwise_logreg`` artifacts are supported (an optional StandardScaler, then a binary
LogisticRegression).  ``pairwise_gbt_phase`` is out of scope.
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


class LearnedWinProbabilityEvaluator:
    """Model-backed evaluator that estimates per-player win probability (the reference's
    surface, plus ``predict_many`` and ``host_probabilities``)."""

    def __init__(self, artifact_path: str, *, max_turns: int = 2500, potential_mode: str = "prob", device: int = 0):
        self.artifact_path = str(artifact_path)
        self.max_turns = int(max_turns)
        self.potential_mode = potential_mode
        self.device = device
        self.model: Optional[WinProbModel] = None
        self._is_dummy = self.artifact_path.endswith("dummy_model.json")
        if self._is_dummy:
            self.model_type = "dummy"
            self.feature_columns: List[str] = []
            return
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
        prob, _, status = self._engine().winprob_eval(pack_states(boards), pack_fsets(boards), None, self.max_turns,
                                                      self.model)
        if status.any():
            bad = int(np.flatnonzero(status)[0])
            raise RuntimeError(f"bk_winprob_eval: board {bad} or its frontier tables are invalid "
                               f"(status {int(status[bad])})")
        return prob

    def host_probabilities(self, rows) -> List[float]:
        """The four probabilities from four feature rows that are already computed (no GPU)."""
        if self._is_dummy:
            return [0.5] * 4
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
