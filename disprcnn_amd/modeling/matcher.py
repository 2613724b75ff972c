"""Matcher: a ground-truth element for every predicted element from their M x N quality matrix (reference: disprcnn/modeling/matcher.py).

    Matcher(high_threshold, low_threshold, allow_low_quality_matches=False)(match_quality_matrix [M,N]) -> matches [N] int64

matches[n] is the row of the largest value of column n (ties: the lowest row), replaced by BELOW_LOW_THRESHOLD (-1) when that value is
below low_threshold and by BETWEEN_THRESHOLDS (-2) when it is below high_threshold.  With allow_low_quality_matches, every prediction
that holds the largest value of some row (ties included) gets its best row back whatever the thresholds say.

Plain torch code.  PointRCNN's training input does its matching in one HIP launch for all images (layers/match2d.py); this class is the
reference's interface and that kernel's comparator in the tests.
"""
import torch


class Matcher(object):
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False):
        if low_threshold > high_threshold:
            raise ValueError("Matcher: low_threshold must not exceed high_threshold")
        self.high_threshold = high_threshold
        self.low_threshold = low_threshold
        self.allow_low_quality_matches = allow_low_quality_matches

    def __call__(self, match_quality_matrix):
        if match_quality_matrix.numel() == 0:
            if match_quality_matrix.shape[0] == 0:
                raise ValueError("No ground-truth boxes available for one of the images during training")
            raise ValueError("No proposal boxes available for one of the images during training")
        matched_vals, matches = match_quality_matrix.max(dim=0)
        all_matches = matches.clone() if self.allow_low_quality_matches else None
        below = matched_vals < self.low_threshold
        between = (matched_vals >= self.low_threshold) & (matched_vals < self.high_threshold)
        matches[below] = Matcher.BELOW_LOW_THRESHOLD
        matches[between] = Matcher.BETWEEN_THRESHOLDS
        if self.allow_low_quality_matches:
            self.set_low_quality_matches_(matches, all_matches, match_quality_matrix)
        return matches

    def set_low_quality_matches_(self, matches, all_matches, match_quality_matrix):
        """Every prediction that has the highest quality of some ground truth (ties included) keeps its best ground truth."""
        highest_per_gt, _ = match_quality_matrix.max(dim=1)
        pairs = torch.nonzero(match_quality_matrix == highest_per_gt[:, None])
        update = pairs[:, 1]
        matches[update] = all_matches[update]
