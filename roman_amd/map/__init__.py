"""roman_amd.map — the part of the reference's mapper (roman.map) that runs on MI355X: the scores of the per-frame data
association and the segment update behind it (§4.26).  Perception, the final clean-up (DBSCAN) and the 2-D mask
IoU of merge() stay in the reference."""
from .association import AssociationParams, association_scores, global_nearest_neighbor  # noqa: F401
from .update import IntegrationParams, IntegrationResult, cleanup_points, integrate  # noqa: F401
