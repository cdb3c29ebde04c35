"""Offline checkpoint comparison of src/evaluate_comparison.py on this build.

The two reference checkpoints (``unet_baseline.pth``, ``unet_pde_regularized.pth``) are loaded
into the HIP ``UNet`` with ``torch.load(..., weights_only=True)`` (state_dict keys and shapes are
the reference's), evaluated on the test folder (per-image Dice / IoU from the fused
kernel's counters, boundary F1 / Hausdorff on the host) and compared with paired tests. Output
files and their columns are the reference's:
  * ``evaluate_and_compare`` (src/evaluate_comparison.py:79-227): evaluation_results_<ts>.csv
    (per image), evaluation_summary_<ts>.csv (per metric), statistical_comparison_<ts>.json;
  * ``run_repeated_evaluations`` (:230-396): aggregated_results_<ts>.csv.
"""
from __future__ import annotations

import json
from datetime import datetime
from pathlib import Path
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .evaluate import (PHYSICS_METRIC_KEYS, PROBABILITY_METRIC_KEYS, SURFACE_METRIC_KEYS, ProbabilityTable,
                       compare_models_statistically, compute_statistics, evaluate_on_test_set, format_metric_report)
from .unet import UNet

METRIC_KEYS = ("dice_scores", "iou_scores", "boundary_f1_scores", "hausdorff_distances")
# appended only when the object-level metrics are switched on (evaluate.py: evaluate_model)
OBJECT_METRIC_KEYS = ("object_f1_scores", "aji_scores", "object_count_errors")
# PROBABILITY_METRIC_KEYS (evaluate.py) likewise, only with the probability-level metrics switched on
_COLUMNS = {"dice_scores": "dice", "iou_scores": "iou", "boundary_f1_scores": "boundary_f1",
            "hausdorff_distances": "hausdorff", "object_f1_scores": "object_f1", "aji_scores": "aji",
            "object_count_errors": "object_count_error", "auroc_scores": "auroc",
            "average_precision_scores": "average_precision", "ece_scores": "ece", "brier_scores": "brier",
            "best_threshold_dice_scores": "best_threshold_dice", "best_thresholds": "best_threshold",
            # PHYSICS_METRIC_KEYS (evaluate.py), only with the physics metrics switched on
            "rd_residuals": "rd_residual", "pf_energies": "pf_energy", "interface_fractions": "interface_fraction",
            # SURFACE_METRIC_KEYS (evaluate.py), only with the surface metrics switched on
            "hausdorff_percentile_distances": "hausdorff_percentile", "assd_distances": "assd",
            "surface_dice_scores": "surface_dice"}
_DEFAULT_OUT = Path(__file__).resolve().parent.parent / "output"


def make_json_serializable(obj: Any) -> Any:
    """numpy scalars/arrays -> Python natives, recursively; anything else unknown -> str
    (src/evaluate_comparison.py:32-58)."""
    if isinstance(obj, np.bool_):
        return bool(obj)
    if isinstance(obj, np.integer):
        return int(obj)
    if isinstance(obj, np.floating):
        return float(obj)
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    if isinstance(obj, dict):
        return {k: make_json_serializable(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [make_json_serializable(v) for v in obj]
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    return str(obj)


def load_model(model_path: Path, device: torch.device) -> UNet:
    """A reference-format checkpoint in the HIP UNet, eval mode (src/evaluate_comparison.py:61-76).
    The file is read with weights_only=True: a checkpoint never executes code here."""
    model = UNet(in_channels=1, out_channels=1, base_channels=64)
    model.load_state_dict(torch.load(model_path, map_location="cpu", weights_only=True))
    return model.to(device).eval()


def _print_comparison(results: Dict[str, Dict[str, float]]):
    print("\nStatistical Test Results (α = 0.05):")
    print("-" * 70)
    for name, r in results.items():
        print(f"\n{name.replace('_', ' ').title()}:")
        if "baseline_mean" not in r:
            print("  fewer than two paired values: no test")
            continue
        print(f"  Baseline Mean: {r['baseline_mean']:.4f}")
        print(f"  PDE Mean:      {r['pde_mean']:.4f}")
        print(f"  Improvement:   {r['improvement']:+.4f}")
        print(f"  Paired t-test:\n    t-statistic: {r['t_statistic']:.4f}\n    p-value:     {r['t_pvalue']:.4f}")
        print(f"  Wilcoxon signed-rank test:\n    statistic:   {r['wilcoxon_statistic']:.4f}\n"
              f"    p-value:     {r['wilcoxon_pvalue']:.4f}")
        print(f"  Significant:  {'Yes' if r['significant'] else 'No'}")


def evaluate_and_compare(baseline_model_path: Path, pde_model_path: Path, test_dir: Path, test_json: Path,
                         device: torch.device, batch_size: int = 8, threshold: float = 0.5,
                         output_dir: Optional[Path] = None, device_cache: bool = False,
                         object_metrics: bool = False, connectivity: int = 8, min_object_area: int = 0,
                         probability_metrics: bool = False, calibration_bins: int = 16,
                         tta: Optional[str] = None, tta_tile: int = 512, tta_overlap: int = 64, refine=None,
                         physics_metrics: bool = False, physics_D: float = 1.0, physics_a: float = 0.5,
                         physics_eps: float = 0.05, surface_metrics: bool = False, surface_percentile: int = 95,
                         surface_tolerance: int = 2) -> Dict:
    """``probability_metrics=True`` adds the six probability-level columns and rows and writes, per
    model, threshold_sweep_<model>_<ts>.csv (the pooled curves, 1024 rows) and
    reliability_<model>_<ts>.csv (``calibration_bins`` rows); the pooled best thresholds go into
    the comparison JSON under "pooled_best_threshold". ``tta`` ("flip" or "d4") evaluates both
    models under test-time augmentation (``evaluate_model``); files and columns do not change.
    ``refine`` (a ``pde.PDERefine``) evolves both models' probabilities under the PDE before every
    metric; ``physics_metrics=True`` adds the three physics columns and rows (``rd_residual``,
    ``pf_energy``, ``interface_fraction``), computed with ``physics_D``, ``physics_a``, ``physics_eps``.
    ``surface_metrics=True`` adds the three surface-distance columns and rows (``hausdorff_percentile`` at
    ``surface_percentile``, ``assd``, ``surface_dice`` at ``surface_tolerance`` pixels)."""
    import pandas as pd
    out_dir = Path(output_dir) if output_dir is not None else _DEFAULT_OUT
    out_dir.mkdir(parents=True, exist_ok=True)
    obj = dict(object_metrics=object_metrics, connectivity=connectivity, min_object_area=min_object_area)
    if tta is not None:
        obj.update(tta=tta, tta_tile=tta_tile, tta_overlap=tta_overlap)
    if refine is not None:
        obj["refine"] = refine
    if physics_metrics:
        obj.update(physics_metrics=True, physics_D=physics_D, physics_a=physics_a, physics_eps=physics_eps)
    if surface_metrics:
        obj.update(surface_metrics=True, surface_percentile=surface_percentile, surface_tolerance=surface_tolerance)
    pooled = {"baseline": ProbabilityTable(), "pde": ProbabilityTable()} if probability_metrics else {}
    prob = {tag: dict(probability_metrics=True, calibration_bins=calibration_bins, probability_table=tab)
            for tag, tab in pooled.items()}
    print("=" * 70 + "\nMODEL EVALUATION AND STATISTICAL COMPARISON\n" + "=" * 70)
    print("\nLoading models...")
    base = evaluate_on_test_set(load_model(baseline_model_path, device), test_dir, test_json, device,
                                batch_size=batch_size, threshold=threshold, model_name="Baseline (Unconstrained)",
                                device_cache=device_cache, **obj, **prob.get("baseline", {}))
    pde = evaluate_on_test_set(load_model(pde_model_path, device), test_dir, test_json, device,
                               batch_size=batch_size, threshold=threshold, model_name="PDE-Constrained",
                               device_cache=device_cache, **obj, **prob.get("pde", {}))
    print("\n" + "=" * 70 + "\nSTATISTICAL COMPARISON\n" + "=" * 70)
    cmp = compare_models_statistically(base, pde, alpha=0.05)
    _print_comparison(cmp)

    ts = datetime.now().strftime("%Y%m%d_%H%M%S")
    per_image = {"image_id": range(len(base["dice_scores"]))}
    for key in (METRIC_KEYS + (OBJECT_METRIC_KEYS if object_metrics else ())
                + (PROBABILITY_METRIC_KEYS if probability_metrics else ())
                + (PHYSICS_METRIC_KEYS if physics_metrics else ())
                + (SURFACE_METRIC_KEYS if surface_metrics else ())):
        col = _COLUMNS[key]
        per_image[f"baseline_{col}"] = base[key]
        per_image[f"pde_{col}"] = pde[key]
    results_csv = out_dir / f"evaluation_results_{ts}.csv"
    pd.DataFrame(per_image).to_csv(results_csv, index=False)
    print(f"\nPer-image metrics saved to: {results_csv}")

    summary = {}
    for name in base:
        sb, sp, c = compute_statistics(base[name]), compute_statistics(pde[name]), cmp[name]
        summary[name] = {"baseline_mean": sb["mean"], "baseline_std": sb["std"], "pde_mean": sp["mean"],
                         "pde_std": sp["std"], "improvement": c.get("improvement", np.nan),
                         "t_pvalue": c["t_pvalue"], "wilcoxon_pvalue": c["wilcoxon_pvalue"],
                         "significant": c["significant"]}
    summary_csv = out_dir / f"evaluation_summary_{ts}.csv"
    pd.DataFrame(summary).T.to_csv(summary_csv)
    print(f"Summary statistics saved to: {summary_csv}")
    comparison_json = out_dir / f"statistical_comparison_{ts}.json"
    payload, files = dict(cmp), {}
    if probability_metrics:
        payload["pooled_best_threshold"] = {}
        for tag, tab in pooled.items():
            thr, dice = tab.best_threshold()
            payload["pooled_best_threshold"][tag] = {"threshold": thr, "dice": dice}
            print(f"Pooled best threshold ({tag}): {thr:.4f} (Dice {dice:.4f})")
            sweep_csv = out_dir / f"threshold_sweep_{tag}_{ts}.csv"
            pd.DataFrame({k: v.cpu().numpy() for k, v in tab.sweep().items()}).to_csv(sweep_csv, index=False)
            reliability_csv = out_dir / f"reliability_{tag}_{ts}.csv"
            rel = {"bin": range(calibration_bins)}
            rel.update({k: v.cpu().numpy() for k, v in tab.reliability(calibration_bins).items()})
            pd.DataFrame(rel).to_csv(reliability_csv, index=False)
            print(f"Threshold sweep and reliability table ({tag}) saved to: {sweep_csv}, {reliability_csv}")
            files[f"threshold_sweep_{tag}_csv"], files[f"reliability_{tag}_csv"] = sweep_csv, reliability_csv
        files["pooled_best_threshold"] = payload["pooled_best_threshold"]
    with open(comparison_json, "w") as f:
        json.dump(make_json_serializable(payload), f, indent=2)
    print(f"Statistical comparison saved to: {comparison_json}")
    return {"baseline_metrics": base, "pde_metrics": pde, "comparison_results": cmp, "results_csv": results_csv,
            "summary_csv": summary_csv, "comparison_json": comparison_json, **files}


def run_repeated_evaluations(baseline_model_paths: List[Path], pde_model_paths: List[Path], test_dir: Path,
                             test_json: Path, device: torch.device, batch_size: int = 8, threshold: float = 0.5,
                             output_dir: Optional[Path] = None, device_cache: bool = False,
                             object_metrics: bool = False, connectivity: int = 8, min_object_area: int = 0,
                             probability_metrics: bool = False, calibration_bins: int = 16,
                             tta: Optional[str] = None, tta_tile: int = 512, tta_overlap: int = 64, refine=None,
                         physics_metrics: bool = False, physics_D: float = 1.0, physics_a: float = 0.5,
                         physics_eps: float = 0.05, surface_metrics: bool = False, surface_percentile: int = 95,
                         surface_tolerance: int = 2) -> Dict:
    """``probability_metrics=True`` adds the six per-image probability-level arrays to the pooled
    statistics (the per-model sweep and reliability files belong to ``evaluate_and_compare``).
    ``tta``, ``refine``, the physics metrics and the surface metrics as ``evaluate_and_compare``."""
    import pandas as pd
    out_dir = Path(output_dir) if output_dir is not None else _DEFAULT_OUT
    out_dir.mkdir(parents=True, exist_ok=True)
    obj = dict(object_metrics=object_metrics, connectivity=connectivity, min_object_area=min_object_area)
    if tta is not None:
        obj.update(tta=tta, tta_tile=tta_tile, tta_overlap=tta_overlap)
    if probability_metrics:
        obj.update(probability_metrics=True, calibration_bins=calibration_bins)
    if refine is not None:
        obj["refine"] = refine
    if physics_metrics:
        obj.update(physics_metrics=True, physics_D=physics_D, physics_a=physics_a, physics_eps=physics_eps)
    if surface_metrics:
        obj.update(surface_metrics=True, surface_percentile=surface_percentile, surface_tolerance=surface_tolerance)
    metric_keys = (METRIC_KEYS + (OBJECT_METRIC_KEYS if object_metrics else ())
                   + (PROBABILITY_METRIC_KEYS if probability_metrics else ())
                   + (PHYSICS_METRIC_KEYS if physics_metrics else ())
                   + (SURFACE_METRIC_KEYS if surface_metrics else ()))
    print("=" * 70 + "\nREPEATED EXPERIMENTS EVALUATION\n" + "=" * 70)
    print(f"Number of runs: {len(baseline_model_paths)}")
    pooled = {"baseline": {k: [] for k in metric_keys}, "pde": {k: [] for k in metric_keys}}
    for i, (bp, pp) in enumerate(zip(baseline_model_paths, pde_model_paths)):
        print(f"\n{'=' * 70}\nRun {i + 1}/{len(baseline_model_paths)}\n{'=' * 70}")
        for tag, path, label in (("baseline", bp, f"Baseline Run {i + 1}"), ("pde", pp, f"PDE-Constrained Run {i + 1}")):
            m = evaluate_on_test_set(load_model(path, device), test_dir, test_json, device, batch_size=batch_size,
                                     threshold=threshold, model_name=label, device_cache=device_cache, **obj)
            for k in metric_keys:
                pooled[tag][k].extend(m[k])
    base = {k: np.array(v) for k, v in pooled["baseline"].items()}
    pde = {k: np.array(v) for k, v in pooled["pde"].items()}
    print("\n" + "=" * 70 + "\nAGGREGATED RESULTS (All Runs Combined)\n" + "=" * 70)
    print(format_metric_report(base, model_name="Baseline (All Runs)"))
    print(format_metric_report(pde, model_name="PDE-Constrained (All Runs)"))
    cmp = compare_models_statistically(base, pde, alpha=0.05)
    print("\n" + "=" * 70 + "\nSTATISTICAL COMPARISON (Aggregated)\n" + "=" * 70)
    for name, r in cmp.items():
        print(f"\n{name.replace('_', ' ').title()}:")
        if "baseline_mean" in r:
            print(f"  Baseline: {r['baseline_mean']:.4f} ± {r.get('baseline_std', 0):.4f}")
            print(f"  PDE:      {r['pde_mean']:.4f} ± {r.get('pde_std', 0):.4f}")
            print(f"  Improvement: {r['improvement']:+.4f}")
        print(f"  Significant: {'Yes' if r['significant'] else 'No'} (p={r['t_pvalue']:.4f})")
    rows = []
    for name in metric_keys:
        for tag, arrs in (("baseline", base), ("pde", pde)):
            st = compute_statistics(arrs[name])
            rows.append({"metric": name, "model": tag, "mean": st["mean"], "std": st["std"], "count": st["count"]})
    aggregated_csv = out_dir / f"aggregated_results_{datetime.now().strftime('%Y%m%d_%H%M%S')}.csv"
    pd.DataFrame(rows, columns=["metric", "model", "mean", "std", "count"]).to_csv(aggregated_csv, index=False)
    print(f"\nAggregated results saved to: {aggregated_csv}")
    return {"baseline_metrics": base, "pde_metrics": pde, "comparison_results": cmp, "aggregated_csv": aggregated_csv}


__all__ = ["METRIC_KEYS", "OBJECT_METRIC_KEYS", "PROBABILITY_METRIC_KEYS", "PHYSICS_METRIC_KEYS", "SURFACE_METRIC_KEYS",
           "make_json_serializable", "load_model", "evaluate_and_compare", "run_repeated_evaluations"]
