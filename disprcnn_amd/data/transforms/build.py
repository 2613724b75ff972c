"""build_transforms(cfg, is_train) of the reference (disprcnn/data/transforms/build.py)."""
from . import transforms as T


def transform_params(cfg, is_train=True):
    """-> (min_size tuple, max_size, flip_prob) the reference reads off cfg.INPUT for training or testing."""
    if is_train:
        min_size, max_size, flip_prob = cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.FLIP_PROB_TRAIN
    else:
        min_size, max_size, flip_prob = cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, 0
    if not isinstance(min_size, (list, tuple)):
        min_size = (min_size,)
    return tuple(min_size), max_size, flip_prob


def build_transforms(cfg, is_train=True):
    min_size, max_size, flip_prob = transform_params(cfg, is_train)
    ts = [
        T.Resize(min_size, max_size),
        T.RandomHorizontalFlip(flip_prob),
        T.ToTensor(),
        T.Normalize(mean=cfg.INPUT.PIXEL_MEAN, std=cfg.INPUT.PIXEL_STD, to_bgr255=cfg.INPUT.TO_BGR255),
    ]
    if not cfg.INPUT.DO_RESIZE:
        ts.pop(0)
    return T.Compose(ts)
