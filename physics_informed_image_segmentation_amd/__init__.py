"""MI355X-native (gfx950) PDE-constrained U-Net segmentation training step.

Drop-in for the hot path of seemapoudel58/Physics_informed_image_segmentation
(src/unet.py, src/pde.py, src/loss.py, src/metrics.py, src/train.py): the
same Python surface, computed by hand-written HIP kernels behind the C-ABI in
include/pis_capi.h. There is no CPU fallback.

Exports the reference package's names (src/__init__.py:35-67) except the four
matplotlib plotting helpers of src/plot.py (out of scope).
"""
__version__ = "0.2.0"

from .dataset import (AffineAugment, CellSegmentationDataset, DeviceCachedLoader, SyntheticDiscDataset,  # noqa: E402
                      pack_samples)
from .evaluate import (ProbabilityTable, best_threshold_batch, boundary_counts,  # noqa: E402
                       compare_models_statistically, compute_aji_batch, compute_assd_batch, compute_auroc_batch,
                       compute_average_precision_batch, compute_boundary_f1, compute_boundary_f1_batch,
                       compute_brier_batch, compute_ece_batch, compute_hausdorff_distance,
                       compute_hausdorff_distance_batch, compute_hausdorff_percentile_batch, compute_iou,
                       compute_iou_batch, compute_object_f1_batch, compute_statistics, compute_surface_dice_batch,
                       distance_transform_sq, distance_transform_sq_np, evaluate_model, evaluate_on_test_set,
                       extract_boundaries_device, format_metric_report, label_components, object_counts,
                       probability_table, surface_distances, threshold_sweep_counts)
from .loss import DiceBCELoss, DiceBCEPDELoss  # noqa: E402
from .metrics import compute_dice_score, compute_dice_score_batch  # noqa: E402
from .optim import AdamW  # noqa: E402
from .pde import (PDELayer, PDERefine, PDERegularization, RefinedModel, create_pde_regularization, energies,  # noqa: E402
                  energies_np, evolve, evolve_np, unroll, unroll_vjp_np, LearnablePDELayer, unroll_coef_vjp_np)
from .train import EarlyStopping, train, train_epoch, train_stage, validate  # noqa: E402
from .unet import UNet, count_parameters  # noqa: E402
from .evaluate_comparison import evaluate_and_compare, run_repeated_evaluations  # noqa: E402
from .ablation import AblationConfig, run_ablation_study, run_ablation_variant  # noqa: E402
from .predict import Predictor, blend_tiles_np, clean_mask, gather_tiles_np, tile_plan  # noqa: E402

__all__ = ["CellSegmentationDataset", "UNet", "DiceBCELoss", "DiceBCEPDELoss", "PDERegularization",
           "create_pde_regularization", "compute_dice_score", "compute_dice_score_batch", "EarlyStopping",
           "train_stage", "validate", "train", "compute_iou", "compute_iou_batch", "compute_boundary_f1",
           "compute_boundary_f1_batch", "compute_hausdorff_distance", "evaluate_model", "evaluate_on_test_set",
           "compare_models_statistically", "format_metric_report", "compute_statistics", "evaluate_and_compare",
           "run_repeated_evaluations", "AblationConfig", "run_ablation_variant", "run_ablation_study",
           # build additions
           "SyntheticDiscDataset", "count_parameters", "train_epoch", "AdamW", "boundary_counts",
           "extract_boundaries_device", "compute_hausdorff_distance_batch", "DeviceCachedLoader", "pack_samples",
           "AffineAugment", "object_counts", "label_components", "compute_object_f1_batch", "compute_aji_batch",
           "probability_table", "threshold_sweep_counts", "compute_auroc_batch", "compute_average_precision_batch",
           "compute_ece_batch", "compute_brier_batch", "best_threshold_batch", "ProbabilityTable",
           "Predictor", "clean_mask", "tile_plan", "gather_tiles_np", "blend_tiles_np",
           "PDERefine", "evolve", "evolve_np", "energies", "energies_np",
           "unroll", "unroll_vjp_np", "PDELayer", "RefinedModel",
           "LearnablePDELayer", "unroll_coef_vjp_np",
           "distance_transform_sq", "distance_transform_sq_np", "surface_distances",
           "compute_hausdorff_percentile_batch", "compute_assd_batch", "compute_surface_dice_batch"]
