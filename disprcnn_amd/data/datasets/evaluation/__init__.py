"""evaluate(dataset, predictions, output_folder, **kwargs) -- reference: disprcnn/data/datasets/evaluation/__init__.py.

The reference dispatches with isinstance on its dataset classes; the dataset classes are not part of this implementation, so the dispatch
goes by the name of the dataset's class (or of one of its bases), which is what a driver that brings its own dataset classes needs."""
from .kitti import kitti_cyclist_evaluation, kitti_evaluation, kitti_pedestrian_evaluation

_BY_CLASS_NAME = {
    "KITTIObjectDatasetCar": kitti_evaluation,
    "KITTIObjectDatasetPedestrian": kitti_pedestrian_evaluation,
    "KITTIObjectDatasetCyclist": kitti_cyclist_evaluation,
}


def evaluate(dataset, predictions, output_folder, **kwargs):
    """evaluate dataset using different methods based on dataset type.
    Args:
        dataset: Dataset object
        predictions(dict(list[BoxList])): 'left' and 'right': the prediction results of each image.
        output_folder: output folder, to save evaluation files or results.
        **kwargs: other args.
    Returns:
        evaluation result
    """
    args = dict(dataset=dataset, left_predictions=predictions["left"], right_predictions=predictions["right"],
                output_folder=output_folder, **kwargs)
    for klass in type(dataset).__mro__:
        if klass.__name__ in _BY_CLASS_NAME:
            return _BY_CLASS_NAME[klass.__name__](**args)
    raise NotImplementedError("Unsupported dataset type {}.".format(dataset.__class__.__name__))
