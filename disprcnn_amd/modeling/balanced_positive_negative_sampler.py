"""BalancedPositiveNegativeSampler (reference: modeling/balanced_positive_negative_sampler.py) on HIP: every image of the batch in one
launch, no host read.

    BalancedPositiveNegativeSampler(batch_size_per_image, positive_fraction)(labels_list, draws=None) -> (pos_masks, neg_masks)

labels_list: per image a tensor of -1 (ignored), 0 (negative) and >= 1 (positive) values, fp32 or int64; the result is the reference's two
lists of uint8 masks.  The randomness is an input (layers/det2d_loss.py:balanced_sample): `draws` is one fp32 uniform in [0, 1) per
candidate of the concatenated lists (one torch.rand call by default), and the candidates with the smallest (draw, index) keys of each
class are taken.  This has the distribution of the reference's randperm(n)[:k], not its generator stream.
"""
import torch

from ..layers.det2d_loss import balanced_sample


class BalancedPositiveNegativeSampler(object):
    def __init__(self, batch_size_per_image, positive_fraction):
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction

    def sample(self, labels, counts, draws=None, want_indices=False):
        """The concatenated form: labels [R] with the images' lengths -> (pos_mask, neg_mask, device counts [N,2], indices)."""
        return balanced_sample(labels, counts, self.batch_size_per_image, self.positive_fraction, draws, want_indices)

    def __call__(self, matched_idxs, draws=None):
        counts = [int(t.shape[0]) for t in matched_idxs]
        pos, neg, _, _ = self.sample(torch.cat(list(matched_idxs), dim=0), counts, draws)
        return list(pos.split(counts)), list(neg.split(counts))
