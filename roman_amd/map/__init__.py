"""roman_amd.map — the part of the reference's mapper (roman.map) that runs on MI355X: the scores of the per-frame data
association.  Perception, the segment update and the 2-D mask IoU of merge() stay in the reference."""
from .association import AssociationParams, association_scores, global_nearest_neighbor  # noqa: F401
