"""d3d_amd.tracking -- the association step of d3d.tracking (reference d3d/tracking/matcher.pyx) on MI355X."""
from .matcher import (DistanceTypes, HungarianMatcher, NearestNeighborMatcher, ScoreMatcher, hungarian_match, linear_sum_assignment,
                      nearest_neighbor_match, prepare_boxes, score_match, score_match_reference_compat)

__all__ = ["DistanceTypes", "ScoreMatcher", "NearestNeighborMatcher", "HungarianMatcher", "prepare_boxes", "score_match",
           "score_match_reference_compat", "nearest_neighbor_match", "hungarian_match", "linear_sum_assignment"]
