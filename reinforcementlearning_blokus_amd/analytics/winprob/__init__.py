"""Win-probability snapshot features (reference: analytics/winprob/)."""
from .features import (SNAPSHOT_FEATURE_COLUMNS, SnapshotRuntimeContext, build_snapshot_runtime_context,
                       coerce_feature_dict, extract_player_snapshot_features, features_from_record,
                       snapshot_features_many)

__all__ = ["SNAPSHOT_FEATURE_COLUMNS", "SnapshotRuntimeContext", "build_snapshot_runtime_context",
           "coerce_feature_dict", "extract_player_snapshot_features", "features_from_record",
           "snapshot_features_many"]
