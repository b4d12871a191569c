"""roman_amd.map — the part of the reference's mapper (roman.map) that runs on MI355X: the scores of the per-frame data
association, the segment update behind it (§4.26) and the final clean-up of a segment that goes inactive (DBSCAN,
§4.27).  Perception and the 2-D mask IoU of merge() stay in the reference."""
from .association import AssociationParams, association_scores, global_nearest_neighbor  # noqa: F401
from .update import (CleanupResult, ClusterParams, IntegrationParams, IntegrationResult, cleanup_points, cluster_labels,  # noqa: F401
                     final_cleanup, integrate, retire)
