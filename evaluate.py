"""Evaluate and compare a baseline and a PDE-constrained checkpoint on the test set — the
reference's eval CLI (evaluate.py:17-146) on the MI355X build: same flags and defaults.

    python evaluate.py --baseline models/unet_baseline.pth --pde models/unet_pde_regularized.pth
    python evaluate.py --baseline 'runs/*/unet_baseline.pth' --pde 'runs/*/unet_pde_regularized.pth' --repeated
"""
import argparse
import os
import sys
from glob import glob
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _calibration_bins(text):
    n = int(text)
    if not 1 <= n <= 1024 or n & (n - 1):
        raise argparse.ArgumentTypeError(f"{text}: a power of two in 1..1024 is needed")
    return n


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate and compare segmentation models")
    ap.add_argument("--baseline", type=str, required=True,
                    help="Path to baseline model checkpoint (or pattern for repeated experiments)")
    ap.add_argument("--pde", type=str, required=True,
                    help="Path to PDE-constrained model checkpoint (or pattern for repeated experiments)")
    ap.add_argument("--test-dir", type=str, default="images/testing",
                    help="Directory containing test images (default: images/testing)")
    ap.add_argument("--test-json", type=str, default="images/annotation/testing_annotation.json",
                    help="Path to test annotations JSON (default: images/annotation/testing_annotation.json)")
    ap.add_argument("--batch-size", type=int, default=8, help="Batch size for evaluation (default: 8)")
    ap.add_argument("--threshold", type=float, default=0.5,
                    help="Threshold for binarizing predictions (default: 0.5)")
    ap.add_argument("--output-dir", type=str, default="output",
                    help="Directory to save evaluation results (default: output)")
    ap.add_argument("--repeated", action="store_true",
                    help="Run repeated experiments evaluation (baseline and pde should be glob patterns)")
    ap.add_argument("--device-cache", action="store_true",
                    help="preprocess the test set once and serve every batch from a device-resident cache")
    ap.add_argument("--augment", choices=["flip", "d4", "affine"], default=None,
                    help="accepted so main.py's data flags can be passed unchanged; it applies to training "
                         "loaders only, and evaluation has none")
    ap.add_argument("--object-metrics", action="store_true",
                    help="also report object-level metrics: detection F1 at IoU > 0.5, Aggregated Jaccard Index "
                         "and the object count error (connected components on the GPU)")
    ap.add_argument("--connectivity", type=int, choices=[4, 8], default=8,
                    help="pixel connectivity of an object for --object-metrics (default: 8)")
    ap.add_argument("--min-object-area", type=int, default=0, metavar="N",
                    help="drop predicted objects below N pixels before --object-metrics (default: 0)")
    ap.add_argument("--probability-metrics", action="store_true",
                    help="also report probability-level metrics: AUROC, average precision, ECE, Brier score and the "
                         "per-image best threshold; writes the pooled threshold sweep and reliability table per model")
    ap.add_argument("--calibration-bins", type=_calibration_bins, default=16, metavar="N",
                    help="confidence bins of the ECE and the reliability table for --probability-metrics: a power "
                         "of two up to 1024 (default: 16)")
    ap.add_argument("--tta", choices=["flip", "d4"], default=None,
                    help="evaluate both models under test-time augmentation: average the predictions over the 4 "
                         "flips or all 8 symmetries of the grid (tiled prediction on the GPU; default: off)")
    from physics_informed_image_segmentation_amd.pde import add_refine_flags, refine_from_args
    add_refine_flags(ap)
    ap.add_argument("--physics-metrics", action="store_true",
                    help="also report per-image physics quantities of the (refined) predictions: the mean squared "
                         "reaction-diffusion residual, the mean phase-field energy and the interface pixel fraction")
    ap.add_argument("--physics-diffusion", type=float, default=1.0, metavar="F",
                    help="diffusion coefficient of the residual for --physics-metrics (default: 1.0)")
    ap.add_argument("--physics-threshold-a", type=float, default=0.5, metavar="F",
                    help="reaction threshold a of the residual for --physics-metrics, in (0, 1) (default: 0.5)")
    ap.add_argument("--physics-epsilon", type=float, default=0.05, metavar="F",
                    help="interface width of the phase-field energy for --physics-metrics (default: 0.05)")
    ap.add_argument("--surface-metrics", action="store_true",
                    help="also report surface-distance metrics: the percentile Hausdorff distance (HD95), the average "
                         "symmetric surface distance and the surface Dice at a tolerance (distance transform on the GPU)")
    ap.add_argument("--surface-percentile", type=int, default=95, metavar="N",
                    help="percentile of the Hausdorff distance for --surface-metrics, 1..100 (default: 95)")
    ap.add_argument("--surface-tolerance", type=int, default=2, metavar="N",
                    help="tolerance in pixels of the surface Dice for --surface-metrics, >= 0 (default: 2)")
    args = ap.parse_args(argv)
    args.refine_preset = refine_from_args(ap, args)
    if args.physics_metrics and not (args.physics_diffusion >= 0 and 0 < args.physics_threshold_a < 1
                                     and args.physics_epsilon > 0):
        ap.error("--physics-metrics: --physics-diffusion >= 0, --physics-threshold-a in (0, 1) and "
                 "--physics-epsilon > 0 are needed")
    if args.surface_metrics and not (1 <= args.surface_percentile <= 100 and 0 <= args.surface_tolerance <= 46340):
        ap.error("--surface-metrics: --surface-percentile in 1..100 and --surface-tolerance in 0..46340 are needed")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    from physics_informed_image_segmentation_amd.evaluate_comparison import (evaluate_and_compare,
                                                                             run_repeated_evaluations)
    # the HIP UNet has no CPU path: evaluation needs the GPU (it raises otherwise)
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    print(f"Using device: {device}")
    common = dict(test_dir=Path(args.test_dir), test_json=Path(args.test_json), device=device,
                  batch_size=args.batch_size, threshold=args.threshold, output_dir=Path(args.output_dir))
    if args.device_cache:
        common["device_cache"] = True
    if args.object_metrics:
        common.update(object_metrics=True, connectivity=args.connectivity, min_object_area=args.min_object_area)
    if args.probability_metrics:
        common.update(probability_metrics=True, calibration_bins=args.calibration_bins)
    if args.tta:
        common["tta"] = args.tta
    if args.refine_preset is not None:
        common["refine"] = args.refine_preset
    if args.physics_metrics:
        common.update(physics_metrics=True, physics_D=args.physics_diffusion, physics_a=args.physics_threshold_a,
                      physics_eps=args.physics_epsilon)
    if args.surface_metrics:
        common.update(surface_metrics=True, surface_percentile=args.surface_percentile,
                      surface_tolerance=args.surface_tolerance)
    if args.repeated:
        base = sorted(glob(args.baseline))
        pde = sorted(glob(args.pde))
        if not base:
            print(f"Error: No baseline models found matching pattern: {args.baseline}")
            return None
        if not pde:
            print(f"Error: No PDE models found matching pattern: {args.pde}")
            return None
        if len(base) != len(pde):
            print(f"Warning: Number of baseline models ({len(base)}) != number of PDE models ({len(pde)})")
        print(f"\nFound {len(base)} baseline models")
        print(f"Found {len(pde)} PDE-constrained models")
        results = run_repeated_evaluations([Path(p) for p in base], [Path(p) for p in pde], **common)
    else:
        bp, pp = Path(args.baseline), Path(args.pde)
        for label, p in (("Baseline", bp), ("PDE", pp)):
            if not p.exists():
                print(f"Error: {label} model not found: {p}")
                return None
        results = evaluate_and_compare(bp, pp, **common)
    print("\n" + "=" * 70 + "\nEVALUATION COMPLETE\n" + "=" * 70)
    return results


if __name__ == "__main__":
    main()
