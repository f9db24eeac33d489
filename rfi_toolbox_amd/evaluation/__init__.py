"""Drop-in for ``rfi_toolbox.evaluation``: segmentation metrics (reference evaluation/metrics.py:25-172) and
flagging-quality statistics (evaluation/statistics.py:10-229)."""
from .detection import (DetectionScorer, InstanceMatch, default_iou_thresholds, match_instances, score_detections,
                        scores_from_matches)
from .metrics import (compute_dice, compute_f1, compute_iou, compute_precision, compute_recall,
                      confusion_counts, evaluate_segmentation)
from .sweep import ThresholdSweep, default_thresholds, sweep_from_counts, threshold_sweep
from .statistics import (compute_calcquality, compute_ffi, compute_statistics, flag_statistics,
                         print_statistics_comparison)

__all__ = ["compute_iou", "compute_precision", "compute_recall", "compute_f1", "compute_dice",
           "evaluate_segmentation", "confusion_counts", "compute_statistics", "compute_ffi", "compute_calcquality",
           "print_statistics_comparison", "flag_statistics", "threshold_sweep", "ThresholdSweep", "sweep_from_counts",
           "default_thresholds", "match_instances", "InstanceMatch", "DetectionScorer", "score_detections", "scores_from_matches",
           "default_iou_thresholds"]
