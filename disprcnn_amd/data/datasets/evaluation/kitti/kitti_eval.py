"""KITTI object evaluation of a list of predictions -- reference: disprcnn/data/datasets/evaluation/kitti/kitti_eval.py.

write_txt writes one KITTI label file per image (utils/kitti_io.kitti_label_lines) and scores them.  Where the reference shells out to the
prebuilt evaluate_object_0.7 / evaluate_object_0.5, this calls layers/kitti_eval.eval_label_dirs, which scores on the GPU with the
overlap table of the program of that name and writes the same stats_<class>_*.txt files next to the label files.  The message is the
reference's ('0.7', 'AP 2d / ori / bev / 3d' of easy, moderate, hard from the 11-point average of every 4th recall sample); it is printed,
and also returned, which the reference does not do.
"""
import os

from .....layers.kitti_eval import eval_label_dirs
from .....utils.kitti_io import kitti_label_lines

PROJECT_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), *[".."] * 5))
DEFAULT_GT_DIR = os.path.join(PROJECT_ROOT, "data/kitti/object/training/label_2")
_MESSAGE_ROWS = (("detection", "2d"), ("orientation", "ori"), ("detection_ground", "bev"), ("detection_3d", "3d"))


def ap_message(iou_thresh, stats):
    """the reference's lines for one program: '%.1f', then 'AP <name> easy moderate hard' for every stats file that exists"""
    msg = "%.1f\n" % iou_thresh
    for key, name in _MESSAGE_ROWS:
        if key in stats:
            ap = (stats[key] * 100)[:, ::4].mean(1).tolist()
            msg += "AP %s %.2f %.2f %.2f\n" % (name, ap[0], ap[1], ap[2])
    return msg


def write_txt(dataset, predictions, output_folder, label="Car", gt_dir=None):
    gt_dir = DEFAULT_GT_DIR if gt_dir is None else gt_dir
    output_folder = os.path.join(output_folder, "txt")
    os.makedirs(output_folder, exist_ok=True)
    for i, prediction in enumerate(predictions):
        imgid = dataset.ids[i]
        size = dataset.infos[int(imgid)]["size"]
        prediction = prediction.resize(size)
        with open(os.path.join(output_folder, imgid + ".txt"), "w") as f:
            f.writelines("\n".join(kitti_label_lines(prediction, label)))
    final_msg = ""
    for iou_thresh in ((0.7, 0.5) if label == "Car" else (0.5,)):
        print(f"-----using iou thresh{iou_thresh}------")
        stats = eval_label_dirs(output_folder, gt_dir, cls=label.lower(), min_overlap=iou_thresh)
        if "detection" not in stats:
            # the reference reads stats_<class>_detection.txt here and fails when the program did not write it
            raise FileNotFoundError(f"no {label} detection to evaluate: stats_{label.lower()}_detection.txt is not written")
        final_msg += ap_message(iou_thresh, stats)
    print(final_msg)
    return final_msg


def do_kitti_evaluation(dataset, left_predictions, right_predictions, class2type, box_only, output_folder, iou_types, expected_results,
                        expected_results_sigma_tol, eval_bbox3d):
    return write_txt(dataset, left_predictions, output_folder)


def do_kitti_pedestrian_evaluation(dataset, left_predictions, right_predictions, class2type, box_only, output_folder, iou_types,
                                   expected_results, expected_results_sigma_tol, eval_bbox3d):
    return write_txt(dataset, left_predictions, output_folder, "Pedestrian")


def do_kitti_cyclist_evaluation(dataset, left_predictions, right_predictions, class2type, box_only, output_folder, iou_types,
                                expected_results, expected_results_sigma_tol, eval_bbox3d):
    return write_txt(dataset, left_predictions, output_folder, "Cyclist")
