"""Evaluation metrics of src/evaluate.py on this build.

* IoU (src/evaluate.py:26-97) is on the hot path (every step, src/train.py:155) and comes
  from the fused loss kernel's exact per-sample counters, like Dice.
* Boundary-F1 and Hausdorff (src/evaluate.py:102-275) are host-side in the reference
  (OpenCV contours + distance transform, scipy Hausdorff). OpenCV is not installed here, so
  they are restated with scipy.ndimage:
    - ``extract_boundaries`` (src/evaluate.py:102-120: cv2.findContours(RETR_EXTERNAL,
      CHAIN_APPROX_NONE) + drawContours(thickness 1)) = the foreground pixels 4-adjacent to
      the OUTER background, i.e. the background component (4-connected, the dual of
      OpenCV's 8-connected foreground) that touches a zero frame around the image. Borders
      of holes and components nested inside holes are not outer contours, as with
      RETR_EXTERNAL.
    - the tolerance test ``distanceTransform(DIST_L2, 5) <= 2`` (:150-175) equals a
      Euclidean-disk test for radius 2 (the 5x5 chamfer gives 1, 1.4, 2 at offsets (1,0),
      (1,1), (2,0) and 2.1969 > 2 at (2,1), exactly where dx^2 + dy^2 <= 4 holds).
    - Hausdorff = scipy's directed_hausdorff both ways on the boundary coordinates (:232-275).
  Parity for these two is unpinned against OpenCV itself (absent); tests/test_host.py pins
  them on hand-drawn shapes with known contours.
* The same two metrics run on the GPU for CUDA tensors (csrc/boundary.hip, pis_boundary_metrics):
  a whole batch per call, a fixed number of launches on the current stream, no host
  synchronisation. Everything in them is integer geometry, so the device path returns the host
  path's boundary maps, counters and squared Hausdorff distances EXACTLY (tests/test_boundary_gpu.py
  compares with ==): outer background by union-find over background pixels with a virtual frame
  node, then per boundary pixel the exact squared distance to the other boundary set from a
  column-distance map. The host dilation tests are Euclidean-disk tests, so one distance pass
  gives both the tolerance counters of boundary F1 and the directed Hausdorff distances.
  ``boundary_counts`` / ``extract_boundaries_device`` / ``compute_hausdorff_distance_batch`` are
  the device entry points; ``compute_boundary_f1_batch``, ``compute_boundary_f1`` and
  ``compute_hausdorff_distance`` take ``backend="auto" | "host" | "device"`` ("auto": device when
  both tensors are CUDA tensors). The host functions are unchanged and are the tests' oracle.
* Object-level metrics (no reference counterpart): connected components of prediction and target,
  detection F1 at IoU > 0.5 / 0.75 and the Aggregated Jaccard Index, from eight exact integer
  counters per sample. ``object_counts`` / ``label_components`` run on the GPU for CUDA tensors
  (csrc/components.hip, pis_object_metrics) and by scipy.ndimage.label + numpy otherwise; the two
  agree with == (tests/test_objects_gpu.py). ``evaluate_model(object_metrics=True)`` adds them.
* Probability-level metrics (no reference counterpart): Dice / IoU at every threshold j / 1024 with
  the best threshold, AUROC, average precision, ECE and the Brier score, all from one exact integer
  table per sample (``probability_table``: csrc/probability.hip, pis_probability_table for CUDA
  tensors, numpy otherwise; == in tests/test_probability_gpu.py). They are the metrics of the
  probabilities rounded up to 16 fractional bits, with thresholds and rank ties on a 1 / 1024 grid.
  ``evaluate_model(probability_metrics=True)`` adds them; ``ProbabilityTable`` pools a loader.
* Surface-distance metrics (no reference counterpart): the exact squared Euclidean distance transform
  (``distance_transform_sq``: csrc/distance.hip, pis_edt_sq for CUDA tensors, scipy otherwise; ==
  in tests/test_surface_gpu.py), the per-pixel distances between the two boundary maps
  (``surface_distances``, pis_surface_distances) and from them the percentile Hausdorff distance
  (HD95), the average symmetric surface distance and the surface Dice at a tolerance.
  ``evaluate_model(surface_metrics=True)`` adds them.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from scipy import ndimage
from scipy.spatial.distance import directed_hausdorff

from . import _hip
from .metrics import compute_dice_score_batch, sample_counts

_FOUR = ndimage.generate_binary_structure(2, 1)
_DISK2 = np.array([[dy * dy + dx * dx <= 4 for dx in range(-2, 3)] for dy in range(-2, 3)])


def compute_iou(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                smooth: float = 1e-6) -> torch.Tensor:
    counts, _ = sample_counts(predictions, targets, threshold, smooth)
    tot = counts.sum(dim=0).to(torch.float32)
    return (tot[0] + smooth) / (tot[1] + tot[2] - tot[0] + smooth)


def compute_iou_batch(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                      smooth: float = 1e-6) -> torch.Tensor:
    return sample_counts(predictions, targets, threshold, smooth)[1][:, 1].contiguous()


def _dilate4(x: np.ndarray, iterations: int = 1) -> np.ndarray:
    """Binary dilation by the 4-neighbour cross (= ndimage.binary_dilation(x, _FOUR)), as
    shifted ORs; two iterations give the Euclidean disk of radius 2 (|dx| + |dy| <= 2 and
    dx^2 + dy^2 <= 4 select the same 13 offsets)."""
    for _ in range(iterations):
        y = x.copy()
        y[1:] |= x[:-1]
        y[:-1] |= x[1:]
        y[:, 1:] |= x[:, :-1]
        y[:, :-1] |= x[:, 1:]
        x = y
    return x


def extract_boundaries(mask: np.ndarray) -> np.ndarray:
    """Outer-contour pixels of a binary (H, W) mask as float32 {0, 1} (src/evaluate.py:102-120)."""
    fg = np.asarray(mask) > 0
    if not fg.any():
        return np.zeros(fg.shape, np.float32)
    pad = np.pad(fg, 1, constant_values=False)
    lab, _ = ndimage.label(~pad, structure=_FOUR)
    outer = lab == lab[0, 0]  # the frame is background and connected to itself
    return (pad & _dilate4(outer))[1:-1, 1:-1].astype(np.float32)


def _near(b: np.ndarray, tolerance: int) -> np.ndarray:
    """Pixels within Euclidean distance ``tolerance`` of a boundary pixel."""
    if tolerance <= 2:
        return _dilate4(b, tolerance)
    disk = np.array([[dy * dy + dx * dx <= tolerance * tolerance for dx in range(-tolerance, tolerance + 1)]
                     for dy in range(-tolerance, tolerance + 1)])
    return ndimage.binary_dilation(b, structure=disk)


def _binary_np(x: torch.Tensor, threshold: float = None) -> np.ndarray:
    a = x.detach().reshape(x.shape[-2], x.shape[-1])
    if threshold is not None:
        a = a > threshold
    return a.cpu().numpy().astype(np.float32)


def _boundary_f1_np(pred_b: np.ndarray, target_b: np.ndarray, tolerance: int, smooth: float) -> float:
    if tolerance > 0:
        near_t = _near(target_b > 0, tolerance)
        near_p = _near(pred_b > 0, tolerance)
        precision = ((near_t * pred_b).sum() + smooth) / (pred_b.sum() + smooth)
        recall = ((near_p * target_b).sum() + smooth) / (target_b.sum() + smooth)
        return float((2.0 * precision * recall + smooth) / (precision + recall + smooth))
    inter = (pred_b * target_b).sum()
    return float((2.0 * inter + smooth) / (pred_b.sum() + target_b.sum() + smooth))

# ----------------------------------------------------------------------------
# Device path (csrc/boundary.hip)
# ----------------------------------------------------------------------------

def _use_device(backend: str, predictions: torch.Tensor, targets: torch.Tensor) -> bool:
    if backend not in ("auto", "host", "device"):
        raise ValueError(f"backend must be 'auto', 'host' or 'device', got {backend!r}")
    both = predictions.is_cuda and targets.is_cuda
    if backend == "device" and not both:
        raise ValueError(f"backend='device' needs CUDA tensors (got {predictions.device}, {targets.device})")
    return both and backend != "host"


def _bhw(x: torch.Tensor) -> torch.Tensor:
    """(B, 1, H, W) / (B, H, W) / (H, W) -> contiguous fp32 (B, H, W)."""
    x = x.detach()
    if x.dim() < 2:
        raise ValueError(f"need (..., H, W), got {tuple(x.shape)}")
    H, W = x.shape[-2], x.shape[-1]
    return x.reshape(-1, H, W).to(torch.float32).contiguous()


def _boundary_device(predictions: torch.Tensor, targets: torch.Tensor, threshold: float, tolerance: int,
                     maps: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """One pis_boundary_metrics call on the current stream: (counts, bnd_p, bnd_t)."""
    p, t = _bhw(predictions), _bhw(targets)
    _hip.require_cuda(p, "boundary_counts")
    _hip.require_cuda(t, "boundary_counts")
    if p.shape != t.shape or p.device != t.device:
        raise ValueError(f"predictions {tuple(p.shape)} on {p.device} and targets {tuple(t.shape)} on {t.device} differ")
    B, H, W = p.shape
    with torch.cuda.device(p.device):
        nbytes = _hip.lib().pis_boundary_ws(B, H, W)
        if nbytes == 0:
            raise ValueError(f"boundary_counts: unsupported shape B={B} H={H} W={W} (B >= 1, 1 <= H, W <= 4096)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
        counts = torch.empty((B, 6), dtype=torch.int32, device=p.device)
        bp = torch.empty((B, H, W), dtype=torch.uint8, device=p.device) if maps else None
        bt = torch.empty((B, H, W), dtype=torch.uint8, device=p.device) if maps else None
        _hip.call("pis_boundary_metrics", _hip.ptr(p), _hip.ptr(t), B, H, W, ctypes.c_float(float(threshold)),
                  int(tolerance), _hip.ptr(counts), _hip.ptr(bp), _hip.ptr(bt), _hip.ptr(ws), nbytes,
                  _hip.stream_handle(p.device))
    return counts, bp, bt


def boundary_counts(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                    tolerance: int = 2) -> torch.Tensor:
    """(B, 6) int32 device tensor (n_p, n_t, m_p, m_t, h2_pt, h2_tp) per sample: boundary sizes,
    boundary pixels within ``tolerance`` of the other boundary, squared directed Hausdorff
    distances (-1 when either boundary is empty). Exact; no host synchronisation."""
    return _boundary_device(predictions, targets, threshold, tolerance)[0]


def extract_boundaries_device(mask_batch: torch.Tensor) -> torch.Tensor:
    """``extract_boundaries`` of every (H, W) mask of a CUDA batch, as uint8 (B, H, W)."""
    return _boundary_device(mask_batch, mask_batch, 0.0, 0, maps=True)[1]


def _f1_from_counts(counts: torch.Tensor, tolerance: int, smooth: float) -> torch.Tensor:
    """``_boundary_f1_np`` on the four counters, float64 on the counters' device."""
    n_p, n_t, m_p, m_t = counts[:, :4].to(torch.float64).unbind(dim=1)
    if tolerance > 0:
        precision = (m_p + smooth) / (n_p + smooth)
        recall = (m_t + smooth) / (n_t + smooth)
        return (2.0 * precision * recall + smooth) / (precision + recall + smooth)
    return (2.0 * m_p + smooth) / (n_p + n_t + smooth)


def _hausdorff_from_counts(counts: torch.Tensor) -> torch.Tensor:
    h2 = torch.maximum(counts[:, 4], counts[:, 5]).to(torch.float64)
    return torch.where(h2 < 0, torch.full_like(h2, float("inf")), h2.clamp_min(0).sqrt())


def compute_hausdorff_distance_batch(predictions: torch.Tensor, targets: torch.Tensor,
                                     threshold: float = 0.5) -> torch.Tensor:
    """Per-sample symmetric Hausdorff distance of the boundaries as a float64 device tensor; inf
    when one boundary is empty. The squared distances are exact integers, so each entry is the
    square root scipy's directed_hausdorff takes."""
    return _hausdorff_from_counts(boundary_counts(predictions, targets, threshold, 0))


def compute_boundary_f1(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                        tolerance: int = 2, smooth: float = 1e-6, backend: str = "auto") -> torch.Tensor:
    """Boundary F1 of the first sample within ``tolerance`` pixels (src/evaluate.py:123-182)."""
    if _use_device(backend, predictions, targets):
        counts = boundary_counts(predictions[0, 0], targets[0, 0], threshold, tolerance)
        return _f1_from_counts(counts, tolerance, smooth)[0].to(torch.float32)
    pb = extract_boundaries(_binary_np(predictions[0, 0], threshold))
    tb = extract_boundaries(_binary_np(targets[0, 0]))
    return torch.tensor(_boundary_f1_np(pb, tb, tolerance, smooth), dtype=torch.float32)


def compute_boundary_f1_batch(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                              tolerance: int = 2, smooth: float = 1e-6, backend: str = "auto") -> torch.Tensor:
    """Per-sample boundary F1 (src/evaluate.py:185-215). Host path: one device->host copy per
    batch, a CPU tensor. Device path: a tensor on the inputs' device, no host synchronisation."""
    if _use_device(backend, predictions, targets):
        return _f1_from_counts(boundary_counts(predictions, targets, threshold, tolerance), tolerance,
                               smooth).to(torch.float32)
    p = (predictions.detach() > threshold).reshape(predictions.shape[0], *predictions.shape[-2:]).cpu().numpy()
    t = targets.detach().reshape(targets.shape[0], *targets.shape[-2:]).cpu().numpy()
    return torch.tensor([_boundary_f1_np(extract_boundaries(p[i]), extract_boundaries(t[i]), tolerance, smooth)
                         for i in range(p.shape[0])], dtype=torch.float32)


def compute_hausdorff_distance(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                               backend: str = "auto") -> float:
    """Symmetric Hausdorff distance of the first sample's boundaries; inf when one is
    empty (src/evaluate.py:218-275)."""
    if _use_device(backend, predictions, targets):
        return float(compute_hausdorff_distance_batch(predictions[0, 0], targets[0, 0], threshold)[0])
    pc = np.column_stack(np.where(extract_boundaries(_binary_np(predictions[0, 0], threshold)) > 0))
    tc = np.column_stack(np.where(extract_boundaries(_binary_np(targets[0, 0])) > 0))
    if len(pc) == 0 or len(tc) == 0:
        return float("inf")
    return float(max(directed_hausdorff(pc, tc)[0], directed_hausdorff(tc, pc)[0]))


# ----------------------------------------------------------------------------
# Object-level metrics: components, detection F1, Aggregated Jaccard Index (csrc/components.hip)
# ----------------------------------------------------------------------------
# Definitions (include/pis_capi.h). An object is a connected component of the
# foreground (prediction: p > threshold, NaN is background; target: t > 0) under ``connectivity``
# (4 or 8); the objects of an image are numbered 1..n in row-major order of their first pixel.
# Predicted objects below ``min_area`` pixels are removed before the numbering and everything
# else; targets are never filtered. The eight counters of a sample are
#   n_p, n_t, tp50 (pairs with 3 I > A_p + A_t), tp75 (7 I > 3 (A_p + A_t)), aji_inter, aji_union,
#   area_p (pixels of the kept predicted objects), removed (predicted objects dropped)
# with AJI in the HoVer-Net form: every true object takes the overlapping prediction of largest
# I / U (exact fractions, ties to the smaller object number); its I and U are added, the
# prediction is marked used; a true object without overlap adds its area to the union, and so
# does every kept prediction that is never used. All integers: the device path equals the host
# path (scipy.ndimage.label + numpy) with ==.

OBJ_NP, OBJ_NT, OBJ_TP50, OBJ_TP75, OBJ_AJI_INTER, OBJ_AJI_UNION, OBJ_AREA_P, OBJ_REMOVED = range(8)
_EIGHT = ndimage.generate_binary_structure(2, 2)


def _check_objects(connectivity: int, min_area: int) -> None:
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 0:
        raise ValueError(f"min_area must be an integer >= 0, got {min_area!r}")


def _label_np(fg: np.ndarray, connectivity: int, min_area: int) -> Tuple[np.ndarray, int, int]:
    """Canonical label map of a boolean (H, W) image: (labels int32, objects kept, objects removed)."""
    lab, n = ndimage.label(fg, structure=_EIGHT if connectivity == 8 else _FOUR)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    ids, first = np.unique(flat[idx], return_index=True)  # the first pixel of every component
    keep = np.bincount(flat, minlength=n + 1)[ids] >= min_area
    ids, first = ids[keep], idx[first[keep]]
    number = np.zeros(n + 1, np.int32)
    number[ids[np.argsort(first, kind="stable")]] = np.arange(1, ids.size + 1, dtype=np.int32)
    return number[lab], int(ids.size), int(n - ids.size)


def _object_counts_np(lp: np.ndarray, n_p: int, removed: int, lt: np.ndarray, n_t: int) -> np.ndarray:
    """The eight counters of one sample from its two canonical label maps."""
    a_p = np.bincount(lp.ravel(), minlength=n_p + 1).astype(np.int64)
    a_t = np.bincount(lt.ravel(), minlength=n_t + 1).astype(np.int64)
    both = (lp > 0) & (lt > 0)
    # pairs sorted by true object, then by predicted object
    code, inter = np.unique(lt[both].astype(np.int64) * (n_p + 1) + lp[both], return_counts=True)
    tt, pp = code // (n_p + 1), code % (n_p + 1)
    inter = inter.astype(np.int64)
    s = a_p[pp] + a_t[tt]
    union = s - inter
    tp50, tp75 = int((3 * inter > s).sum()), int((7 * inter > 3 * s).sum())
    used = np.zeros(n_p + 1, bool)
    matched = np.zeros(n_t + 1, bool)
    aji_i = aji_u = 0
    _, start, size = np.unique(tt, return_index=True, return_counts=True)
    for b, k in zip(start.tolist(), size.tolist()):
        best = b
        for e in range(b + 1, b + k):  # ascending object number: '>' leaves ties with the smaller
            if int(inter[e]) * int(union[best]) > int(inter[best]) * int(union[e]):
                best = e
        aji_i += int(inter[best])
        aji_u += int(union[best])
        used[pp[best]] = True
        matched[tt[best]] = True
    aji_u += int(a_t[1:][~matched[1:]].sum()) + int(a_p[1:][~used[1:]].sum())
    return np.array([n_p, n_t, tp50, tp75, aji_i, aji_u, int(a_p[1:].sum()), removed], np.int64)


def _objects_host(predictions: torch.Tensor, targets: torch.Tensor, threshold: float, connectivity: int,
                  min_area: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(counts (B, 8) int64, labels_p, labels_t (B, H, W) int32) by scipy and numpy."""
    p, t = _bhw(predictions).cpu().numpy(), _bhw(targets).cpu().numpy()
    if p.shape != t.shape:
        raise ValueError(f"predictions {p.shape} and targets {t.shape} differ")
    counts, lps, lts = [], [], []
    with np.errstate(invalid="ignore"):
        fp, ft = p > threshold, t > 0
    for i in range(p.shape[0]):
        lp, n_p, removed = _label_np(fp[i], connectivity, min_area)
        lt, n_t, _ = _label_np(ft[i], connectivity, 0)
        counts.append(_object_counts_np(lp, n_p, removed, lt, n_t))
        lps.append(lp)
        lts.append(lt)
    return np.stack(counts), np.stack(lps), np.stack(lts)


def _objects_device(predictions: torch.Tensor, targets: torch.Tensor, threshold: float, connectivity: int,
                    min_area: int, maps: bool = False, ws: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """One pis_object_metrics call on the current stream: (counts, labels_p, labels_t). ``ws``: a
    uint8 CUDA tensor of at least pis_objects_ws bytes to use as the workspace (its contents do not
    matter); allocated from the caching allocator when None."""
    p, t = _bhw(predictions), _bhw(targets)
    _hip.require_cuda(p, "object_counts")
    _hip.require_cuda(t, "object_counts")
    if p.shape != t.shape or p.device != t.device:
        raise ValueError(f"predictions {tuple(p.shape)} on {p.device} and targets {tuple(t.shape)} on {t.device} differ")
    B, H, W = p.shape
    with torch.cuda.device(p.device):
        nbytes = _hip.lib().pis_objects_ws(B, H, W)
        if nbytes == 0:
            raise ValueError(f"object_counts: unsupported shape B={B} H={H} W={W} (B >= 1, 1 <= H, W <= 4096)")
        if ws is None:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
        counts = torch.empty((B, 8), dtype=torch.int64, device=p.device)
        lp = torch.empty((B, H, W), dtype=torch.int32, device=p.device) if maps else None
        lt = torch.empty((B, H, W), dtype=torch.int32, device=p.device) if maps else None
        _hip.call("pis_object_metrics", _hip.ptr(p), _hip.ptr(t), B, H, W, ctypes.c_float(float(threshold)),
                  int(connectivity), int(min_area), _hip.ptr(counts), _hip.ptr(lp), _hip.ptr(lt), _hip.ptr(ws),
                  ws.numel(), _hip.stream_handle(p.device))
    return counts, lp, lt


def object_counts(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5, connectivity: int = 8,
                  min_area: int = 0, backend: str = "auto") -> torch.Tensor:
    """(B, 8) int64 (n_p, n_t, tp50, tp75, aji_inter, aji_union, area_p, removed) per sample. CUDA
    tensors: on their device, one pis_object_metrics call, no host synchronisation. CPU tensors
    (and ``backend="host"``): scipy.ndimage.label + numpy, a CPU tensor; the two agree exactly."""
    _check_objects(connectivity, min_area)
    if _use_device(backend, predictions, targets):
        return _objects_device(predictions, targets, threshold, connectivity, int(min_area))[0]
    return torch.from_numpy(_objects_host(predictions, targets, threshold, connectivity, int(min_area))[0])


def label_components(masks: torch.Tensor, threshold: float = 0.0, connectivity: int = 8, min_area: int = 0,
                     backend: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """Objects of every (H, W) image of a batch (foreground: mask > threshold): (labels int32
    (B, H, W), n int64 (B,)), numbered 1..n in row-major order of their first pixel; 0 is the
    background and every object below ``min_area`` pixels."""
    _check_objects(connectivity, min_area)
    if _use_device(backend, masks, masks):
        counts, lp, _ = _objects_device(masks, masks, threshold, connectivity, int(min_area), maps=True)
        return lp, counts[:, OBJ_NP].contiguous()
    with np.errstate(invalid="ignore"):
        fg = _bhw(masks).cpu().numpy() > threshold
    res = [_label_np(m, connectivity, int(min_area)) for m in fg]
    return (torch.from_numpy(np.stack([r[0] for r in res])),
            torch.tensor([r[1] for r in res], dtype=torch.int64))


def _object_f1_from_counts(counts: torch.Tensor, iou: float = 0.5) -> torch.Tensor:
    """2 tp / (n_p + n_t) as float64 on the counters' device; NaN where there is no object at all."""
    if iou not in (0.5, 0.75):
        raise ValueError(f"iou must be 0.5 or 0.75, got {iou!r}")
    c = counts.to(torch.float64)
    den = c[:, OBJ_NP] + c[:, OBJ_NT]
    f1 = 2.0 * c[:, OBJ_TP50 if iou == 0.5 else OBJ_TP75] / den
    return torch.where(den > 0, f1, torch.full_like(f1, float("nan")))


def _aji_from_counts(counts: torch.Tensor) -> torch.Tensor:
    c = counts.to(torch.float64)
    aji = c[:, OBJ_AJI_INTER] / c[:, OBJ_AJI_UNION]
    return torch.where(c[:, OBJ_NP] + c[:, OBJ_NT] > 0, aji, torch.full_like(aji, float("nan")))


def compute_object_f1_batch(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                            connectivity: int = 8, min_area: int = 0, iou: float = 0.5,
                            backend: str = "auto") -> torch.Tensor:
    """Per-sample detection F1 at IoU > ``iou`` (0.5 or 0.75): 2 tp / (n_p + n_t), float64 on the
    counters' device; NaN for a sample with no predicted and no true object."""
    if iou not in (0.5, 0.75):
        raise ValueError(f"iou must be 0.5 or 0.75, got {iou!r}")
    return _object_f1_from_counts(object_counts(predictions, targets, threshold, connectivity, min_area, backend), iou)


def compute_aji_batch(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                      connectivity: int = 8, min_area: int = 0, backend: str = "auto") -> torch.Tensor:
    """Per-sample Aggregated Jaccard Index aji_inter / aji_union, float64 on the counters' device;
    NaN for a sample with no predicted and no true object."""
    return _aji_from_counts(object_counts(predictions, targets, threshold, connectivity, min_area, backend))


# ----------------------------------------------------------------------------
# Probability-level metrics: threshold sweep, AUROC, average precision, ECE, Brier
# (csrc/probability.hip)
# ----------------------------------------------------------------------------
# Definitions (include/pis_capi.h). Everything derives from one integer table per
# sample. Per pixel, with every float step exact in fp32:
#   x = p * 65536;  q = clamp(ceil(x), 0, 65536) (NaN: 0, counted in n_nan);  bin = (q + 63) >> 6
#   cls = t > 0.5 (the target test of the Dice / IoU counters; a NaN target is class 0)
#   table[b][cls][bin] = (count, sum of q);  extra[b] = (sum q^2 class 0, sum q^2 class 1, n_nan, 0)
# so that p > j / 1024 holds exactly when bin > j (j = 0..1023; strict, NaN is background). The
# scores below are torch integer arithmetic on that table up to one final float64 division, the
# same code for the device path (pis_probability_table) and the host path (numpy): the two tables
# agree with ==. What is quantised: all scores are those of the probabilities rounded UP to 16
# fractional bits; thresholds lie on the 10-bit grid j / 1024; AUROC and average precision treat
# the pixels of one 1 / 1024 bin as tied.

PROB_BINS, PROB_QBITS = 1024, 16
PROB_ONE = 1 << PROB_QBITS
PROB_BLOCK_PIXELS = 8192  # csrc/probability.hip PB_PIX: the pixels one block of the histogram kernel counts
PROB_NEG, PROB_POS = 0, 1


def _check_calibration_bins(n_bins: int) -> int:
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 1 <= n_bins <= PROB_BINS \
            or n_bins & (n_bins - 1):
        raise ValueError(f"n_bins must be a power of two in 1..{PROB_BINS}, got {n_bins!r}")
    return int(n_bins)


def _probability_host(predictions: torch.Tensor, targets: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """(table (B, 2, 1025, 2) int64, extra (B, 4) int64) by numpy, from the definitions above."""
    p, t = _bhw(predictions).cpu().numpy(), _bhw(targets).cpu().numpy()
    if p.shape != t.shape:
        raise ValueError(f"predictions {p.shape} and targets {t.shape} differ")
    B = p.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        x = p * np.float32(PROB_ONE)
        # p > 0 is False for NaN, -Inf, negatives and both zeros: q = 0. A positive p whose x
        # underflows still has ceil(x) = 1.
        q = np.where(p > 0, np.clip(np.ceil(x), 1, PROB_ONE), 0).astype(np.int64)
        cls = (t > np.float32(0.5)).astype(np.int64)
    key = (cls * (PROB_BINS + 1) + ((q + 63) >> 6)).reshape(B, -1)
    q, cls, nan = q.reshape(B, -1), cls.reshape(B, -1), np.isnan(p).reshape(B, -1)
    table = np.zeros((B, 2 * (PROB_BINS + 1), 2), np.int64)
    extra = np.zeros((B, 4), np.int64)
    for b in range(B):
        table[b, :, 0] = np.bincount(key[b], minlength=2 * (PROB_BINS + 1))
        # float64 weights: every partial sum is an integer below 2^40, exact
        table[b, :, 1] = np.bincount(key[b], weights=q[b].astype(np.float64), minlength=2 * (PROB_BINS + 1))
        q2 = q[b] * q[b]
        extra[b, 0], extra[b, 1], extra[b, 2] = q2[cls[b] == 0].sum(), q2[cls[b] == 1].sum(), nan[b].sum()
    return table.reshape(B, 2, PROB_BINS + 1, 2), extra


def _probability_device(predictions: torch.Tensor, targets: torch.Tensor, ws: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pis_probability_table call (two launches) on the current stream: (table, extra). ``ws``:
    a uint8 CUDA tensor of at least pis_probability_ws bytes to use as the workspace (its contents
    do not matter); allocated from the caching allocator when None."""
    p, t = _bhw(predictions), _bhw(targets)
    _hip.require_cuda(p, "probability_table")
    _hip.require_cuda(t, "probability_table")
    if p.shape != t.shape or p.device != t.device:
        raise ValueError(f"predictions {tuple(p.shape)} on {p.device} and targets {tuple(t.shape)} on {t.device} differ")
    B, H, W = p.shape
    with torch.cuda.device(p.device):
        nbytes = _hip.lib().pis_probability_ws(B, H, W)
        if nbytes == 0:
            raise ValueError(f"probability_table: unsupported shape B={B} H={H} W={W} (B >= 1, 1 <= H, W <= 4096)")
        if ws is None:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
        table = torch.empty((B, 2, PROB_BINS + 1, 2), dtype=torch.int64, device=p.device)
        extra = torch.empty((B, 4), dtype=torch.int64, device=p.device)
        _hip.call("pis_probability_table", _hip.ptr(p), _hip.ptr(t), B, H, W, _hip.ptr(table), _hip.ptr(extra),
                  _hip.ptr(ws), ws.numel(), _hip.stream_handle(p.device))
    return table, extra


def probability_table(predictions: torch.Tensor, targets: torch.Tensor, backend: str = "auto"
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(table (B, 2, 1025, 2) int64, extra (B, 4) int64) of a (B, H, W) or (B, 1, H, W) batch:
    ``table[b, cls, bin] = (count, sum of q)`` and ``extra[b] = (sum q^2 over class 0, over class 1,
    n_nan, 0)`` with q the probability rounded UP to 16 fractional bits, bin = ceil(p * 1024) clamped to
    0..1024 and cls = t > 0.5. CUDA tensors: on their device, one pis_probability_table call, no host
    synchronisation. CPU tensors (and ``backend="host"``): numpy, CPU tensors; the two agree exactly."""
    if _use_device(backend, predictions, targets):
        return _probability_device(predictions, targets)
    table, extra = _probability_host(predictions, targets)
    return torch.from_numpy(table), torch.from_numpy(extra)


def _as_table(a, b, backend: str, need_extra: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(predictions, targets) -> their table; a table, or a (table, extra) pair, passes through."""
    if b is None:
        table, extra = a if isinstance(a, (tuple, list)) else (a, None)
    else:
        table, extra = probability_table(a, b, backend)
    if table.dtype != torch.int64 or table.dim() != 4 or tuple(table.shape[1:]) != (2, PROB_BINS + 1, 2):
        raise ValueError(f"need an int64 table of shape (B, 2, {PROB_BINS + 1}, 2), got {table.dtype} "
                         f"{tuple(table.shape)} (or pass predictions and targets)")
    if need_extra and (extra is None or extra.dtype != torch.int64 or tuple(extra.shape) != (table.shape[0], 4)):
        raise ValueError("the Brier score needs (table, extra) as returned by probability_table")
    return table, extra


def _nan_where(cond: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return torch.where(cond, torch.full_like(x, float("nan")), x)


def _suffix_sum(x: torch.Tensor) -> torch.Tensor:
    """out[..., i] = sum over k >= i of x[..., k]."""
    return x.flip(-1).cumsum(-1).flip(-1)


def threshold_sweep_counts(table: torch.Tensor) -> torch.Tensor:
    """(B, 1024, 3) int64 ``(I_hat, P_hat, T)`` at the thresholds j / 1024, j = 0..1023, from a table:
    the counters ``sample_counts(p, t, j / 1024)`` returns (row 512: threshold 0.5). Exact."""
    table, _ = _as_table(table, None, "auto")
    pos, neg = table[:, PROB_POS, :, 0], table[:, PROB_NEG, :, 0]
    i_hat = _suffix_sum(pos)[:, 1:]              # bins above j
    p_hat = _suffix_sum(pos + neg)[:, 1:]
    return torch.stack([i_hat, p_hat, pos.sum(-1, keepdim=True).expand_as(i_hat)], dim=-1)


def _sweep_scores(counts: torch.Tensor, smooth: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Dice, IoU) per threshold in float64 by the formulas of the fused counters."""
    i_hat, p_hat, t = counts.to(torch.float64).unbind(-1)
    return (2.0 * i_hat + smooth) / (p_hat + t + smooth), (i_hat + smooth) / (p_hat + t - i_hat + smooth)


def best_threshold_batch(predictions, targets=None, backend: str = "auto", smooth: float = 1e-6
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per sample the first threshold j / 1024 that maximises the Dice score, and that score: two
    float64 tensors on the table's device. Takes (predictions, targets) or a table."""
    table, _ = _as_table(predictions, targets, backend)
    dice, _ = _sweep_scores(threshold_sweep_counts(table), smooth)
    j = torch.argmax(dice, dim=1)  # the first maximum
    return j.to(torch.float64) / PROB_BINS, dice.gather(1, j[:, None])[:, 0]


def compute_auroc_batch(predictions, targets=None, backend: str = "auto") -> torch.Tensor:
    """Per-sample area under the ROC curve of the 1025-bin ranking, float64 on the table's device:
    sum_i pos_i (2 below_i + neg_i) / (2 P Nn), the pixels of one 1 / 1024 bin counted as ties (half).
    NaN for a sample without positives or without negatives. Takes (predictions, targets) or a table."""
    table, _ = _as_table(predictions, targets, backend)
    pos, neg = table[:, PROB_POS, :, 0], table[:, PROB_NEG, :, 0]
    below = neg.cumsum(-1) - neg
    num = (pos * (2 * below + neg)).sum(-1)        # below 2^50
    den = 2 * pos.sum(-1) * neg.sum(-1)
    return _nan_where(den == 0, num.to(torch.float64) / den.to(torch.float64))


def compute_average_precision_batch(predictions, targets=None, backend: str = "auto") -> torch.Tensor:
    """Per-sample average precision in the step form over the bins from 1024 down to 0:
    sum_i (pos_i / P) (TP_i / PP_i) with TP_i, PP_i the positives / all pixels in bins >= i (terms
    with PP_i = 0 are empty). float64; NaN for a sample without positives."""
    table, _ = _as_table(predictions, targets, backend)
    pos, neg = table[:, PROB_POS, :, 0], table[:, PROB_NEG, :, 0]
    tp, pp = _suffix_sum(pos), _suffix_sum(pos + neg)
    p_all = pos.sum(-1, keepdim=True)
    den = p_all * pp
    terms = (pos * tp).to(torch.float64) / den.clamp_min(1).to(torch.float64)   # pos_i = 0 where den = 0
    return _nan_where(p_all[:, 0] == 0, terms.sum(-1))


def _coarse_bins(table: torch.Tensor, n_bins: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(count, positives, sum of q) per coarse bin, (B, n_bins) int64 each: coarse bin m holds the
    fine bins i with (i - 1) // (1024 / n_bins) == m, and fine bin 0 (q = 0) joins m = 0."""
    both = table[:, PROB_NEG] + table[:, PROB_POS]                      # (B, 1025, 2)
    B = table.shape[0]

    def fold(x):
        y = x[:, 1:].reshape(B, n_bins, PROB_BINS // n_bins).sum(-1)
        y[:, 0] += x[:, 0]
        return y
    return fold(both[..., 0]), fold(table[:, PROB_POS, :, 0]), fold(both[..., 1])


def compute_ece_batch(predictions, targets=None, n_bins: int = 16, backend: str = "auto") -> torch.Tensor:
    """Per-sample expected calibration error with ``n_bins`` equal-width confidence bins (a power of
    two up to 1024): sum_m |SQ_m - 65536 pos_m| / (65536 N), i.e. sum_m (n_m / N) |mean confidence -
    positive fraction| of the probabilities rounded up to 16 bits. float64."""
    n_bins = _check_calibration_bins(n_bins)
    table, _ = _as_table(predictions, targets, backend)
    count, pos, sq = _coarse_bins(table, n_bins)
    num = (sq - PROB_ONE * pos).abs().sum(-1)
    return num.to(torch.float64) / (PROB_ONE * count.sum(-1)).to(torch.float64)


def compute_brier_batch(predictions, targets=None, backend: str = "auto") -> torch.Tensor:
    """Per-sample Brier score mean((q / 65536 - cls)^2) from the integer sums:
    (S2_neg + S2_pos - 2 * 65536 SQ_pos + 2^32 P) / (2^32 N). float64. Takes (predictions, targets)
    or the pair (table, extra)."""
    table, extra = _as_table(predictions, targets, backend, need_extra=True)
    pos = table[:, PROB_POS]
    n = table[..., 0].sum((1, 2))
    num = extra[:, 0] + extra[:, 1] - 2 * PROB_ONE * pos[..., 1].sum(-1) + (PROB_ONE * PROB_ONE) * pos[..., 0].sum(-1)
    return num.to(torch.float64) / ((PROB_ONE * PROB_ONE) * n).to(torch.float64)


class ProbabilityTable:
    """The pooled table of a whole loader: ``update`` adds every sample of a batch's table (on the
    table's device; integers, so pooling is exact and does not depend on the order), and the pooled
    curves and scores come from the sums by the same arithmetic as the per-sample ones."""

    def __init__(self):
        self.table: Optional[torch.Tensor] = None   # (2, 1025, 2) int64
        self.extra: Optional[torch.Tensor] = None   # (4,) int64

    def update(self, table: torch.Tensor, extra: torch.Tensor) -> "ProbabilityTable":
        table, extra = _as_table((table, extra), None, "auto", need_extra=True)
        if self.table is None:
            self.table, self.extra = table.sum(0), extra.sum(0)
        else:
            self.table += table.sum(0).to(self.table.device)
            self.extra += extra.sum(0).to(self.extra.device)
        return self

    def _batch(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.table is None:
            raise ValueError("ProbabilityTable: no batch has been added yet")
        return self.table[None], self.extra[None]

    @property
    def total_count(self) -> int:
        return 0 if self.table is None else int(self.table[..., 0].sum())

    def sweep(self) -> Dict[str, torch.Tensor]:
        """Pooled per-threshold curves, 1024 rows: ``threshold`` j / 1024, ``tp``, ``fp``, ``fn``
        (int64), ``precision`` (NaN where nothing is predicted), ``recall`` (NaN without positives),
        ``dice`` and ``iou`` (the smoothed formulas of the per-image scores), float64."""
        c = threshold_sweep_counts(self._batch()[0])[0]
        tp, fp, fn = c[:, 0], c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        dice, iou = _sweep_scores(c)
        f = torch.float64
        return {"threshold": torch.arange(PROB_BINS, dtype=f, device=c.device) / PROB_BINS, "tp": tp, "fp": fp,
                "fn": fn, "precision": _nan_where(c[:, 1] == 0, tp.to(f) / c[:, 1].to(f)),
                "recall": _nan_where(c[:, 2] == 0, tp.to(f) / c[:, 2].to(f)), "dice": dice, "iou": iou}

    def best_threshold(self) -> Tuple[float, float]:
        """(threshold, Dice): the first threshold j / 1024 that maximises the pooled Dice score."""
        thr, dice = best_threshold_batch(self._batch()[0])
        return float(thr[0]), float(dice[0])

    def reliability(self, n_bins: int = 16) -> Dict[str, torch.Tensor]:
        """Per confidence bin (``n_bins`` equal-width bins, a power of two up to 1024): ``count``
        (int64), ``mean_confidence`` and ``positive_fraction`` (float64, NaN for an empty bin)."""
        n_bins = _check_calibration_bins(n_bins)
        count, pos, sq = (x[0] for x in _coarse_bins(self._batch()[0], n_bins))
        f = torch.float64
        return {"count": count, "mean_confidence": _nan_where(count == 0, sq.to(f) / (PROB_ONE * count).to(f)),
                "positive_fraction": _nan_where(count == 0, pos.to(f) / count.to(f))}

    def auroc(self) -> float:
        return float(compute_auroc_batch(self._batch()[0])[0])

    def average_precision(self) -> float:
        return float(compute_average_precision_batch(self._batch()[0])[0])

    def ece(self, n_bins: int = 16) -> float:
        return float(compute_ece_batch(self._batch()[0], n_bins=n_bins)[0])

    def brier(self) -> float:
        return float(compute_brier_batch(self._batch())[0])


# ----------------------------------------------------------------------------
# Distance transform and surface-distance metrics: HD95, ASSD, surface Dice (csrc/distance.hip)
# ----------------------------------------------------------------------------
# Definitions (include/pis_capi.h). The squared Euclidean distance transform of a set is,
# per pixel, the smallest (y - y')^2 + (x - x')^2 over the set's pixels: an exact int32, 0 inside the
# set, EDT_NONE everywhere when the set is empty. With Bp, Bt the boundary maps of a sample
# (``extract_boundaries`` of p > threshold and of t > 0), the surface distances are the two tables
#   d2_pt[q] = the transform of Bt at q for q in Bp, -1 elsewhere;  d2_tp the mirror image
# and the three scores are torch arithmetic on them (the same code for both backends):
#   Hausdorff percentile  per direction the nearest-rank percentile of the n distances, the
#                         k-th smallest with k = (percentile n + 99) // 100; sqrt of the larger one
#   ASSD                  (sum_Bp sqrt(d2_pt) + sum_Bt sqrt(d2_tp)) / (n_p + n_t)
#   surface Dice          (m_p + m_t + smooth) / (n_p + n_t + smooth), m = #[0 <= d2 <= tolerance^2]
# The first two are inf when either boundary is empty, as compute_hausdorff_distance is.

EDT_NONE = 2 ** 31 - 1
# the per-image arrays evaluate_model(surface_metrics=True) adds, in this order
SURFACE_METRIC_KEYS = ("hausdorff_percentile_distances", "assd_distances", "surface_dice_scores")


def _check_backend(backend: str) -> None:
    if backend not in ("auto", "host", "device"):
        raise ValueError(f"backend must be 'auto', 'host' or 'device', got {backend!r}")


def _check_percentile(percentile: int) -> int:
    if isinstance(percentile, bool) or not isinstance(percentile, (int, np.integer)) or not 1 <= percentile <= 100:
        raise ValueError(f"percentile must be an integer in 1..100, got {percentile!r}")
    return int(percentile)


def _check_surface_tolerance(tolerance: int) -> int:
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, np.integer)) or not 0 <= tolerance <= 46340:
        raise ValueError(f"tolerance must be an integer in 0..46340, got {tolerance!r}")
    return int(tolerance)


def distance_transform_sq_np(mask: np.ndarray) -> np.ndarray:
    """The definition of record: the squared Euclidean distance transform of every (H, W) image of
    ``mask`` ((..., H, W); the set is ``mask > 0``, so NaN is outside) as int32 (B, H, W), by
    scipy.ndimage.distance_transform_edt, squared and rounded (exact: the squares are integers far
    below 2^53). An image with an empty set is EDT_NONE everywhere."""
    a = np.asarray(mask)
    if a.ndim < 2:
        raise ValueError(f"need (..., H, W), got {a.shape}")
    with np.errstate(invalid="ignore"):
        s = a.reshape(-1, a.shape[-2], a.shape[-1]) > 0
    out = np.full(s.shape, EDT_NONE, np.int32)
    for i, m in enumerate(s):
        if m.any():
            out[i] = np.rint(ndimage.distance_transform_edt(~m) ** 2).astype(np.int32)
    return out


def _edt_device(sets: torch.Tensor) -> torch.Tensor:
    """One pis_edt_sq call (three launches) on the current stream; ``sets``: uint8 (B, H, W) on the GPU."""
    _hip.require_cuda(sets, "distance_transform_sq")
    B, H, W = sets.shape
    with torch.cuda.device(sets.device):
        nbytes = _hip.lib().pis_edt_ws(B, H, W)
        if nbytes == 0:
            raise ValueError(f"distance_transform_sq: unsupported shape B={B} H={H} W={W} (B >= 1, 1 <= H, W <= 4096)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=sets.device)
        d2 = torch.empty((B, H, W), dtype=torch.int32, device=sets.device)
        _hip.call("pis_edt_sq", _hip.ptr(sets), B, H, W, _hip.ptr(d2), _hip.ptr(ws), nbytes,
                  _hip.stream_handle(sets.device))
    return d2


def distance_transform_sq(mask: torch.Tensor, backend: str = "auto") -> torch.Tensor:
    """Squared Euclidean distance from every pixel to the nearest pixel of the set ``mask > 0`` of
    its image, int32 (B, H, W) for a (B, 1, H, W), (B, H, W) or (H, W) input: 0 inside the set,
    EDT_NONE for an image with an empty set. CUDA tensors: on their device, one pis_edt_sq call, no
    host synchronisation. CPU tensors (and ``backend="host"``): ``distance_transform_sq_np``, a CPU
    tensor; the two agree exactly."""
    if _use_device(backend, mask, mask):
        m = mask.detach()
        if m.dim() < 2:
            raise ValueError(f"need (..., H, W), got {tuple(m.shape)}")
        return _edt_device((m.reshape(-1, m.shape[-2], m.shape[-1]) > 0).to(torch.uint8).contiguous())
    return torch.from_numpy(distance_transform_sq_np(_bhw(mask).cpu().numpy()))


def _surface_host(predictions: torch.Tensor, targets: torch.Tensor, threshold: float) -> Tuple[np.ndarray, np.ndarray]:
    p, t = _bhw(predictions).cpu().numpy(), _bhw(targets).cpu().numpy()
    if p.shape != t.shape:
        raise ValueError(f"predictions {p.shape} and targets {t.shape} differ")
    with np.errstate(invalid="ignore"):
        fp, ft = p > threshold, t > 0
    bp = np.stack([extract_boundaries(m) for m in fp]) > 0
    bt = np.stack([extract_boundaries(m) for m in ft]) > 0
    return (np.where(bp, distance_transform_sq_np(bt), np.int32(-1)),
            np.where(bt, distance_transform_sq_np(bp), np.int32(-1)))


def _surface_device(predictions: torch.Tensor, targets: torch.Tensor, threshold: float
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pis_boundary_metrics call for the two boundary maps, one pis_surface_distances call."""
    _, bp, bt = _boundary_device(predictions, targets, threshold, 0, maps=True)
    B, H, W = bp.shape
    with torch.cuda.device(bp.device):
        nbytes = _hip.lib().pis_surface_distances_ws(B, H, W)
        if nbytes == 0:
            raise ValueError(f"surface_distances: unsupported shape B={B} H={H} W={W} (B >= 1, 1 <= H, W <= 4096)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=bp.device)
        d2_pt = torch.empty((B, H, W), dtype=torch.int32, device=bp.device)
        d2_tp = torch.empty((B, H, W), dtype=torch.int32, device=bp.device)
        _hip.call("pis_surface_distances", _hip.ptr(bp), _hip.ptr(bt), B, H, W, _hip.ptr(d2_pt), _hip.ptr(d2_tp),
                  _hip.ptr(ws), nbytes, _hip.stream_handle(bp.device))
    return d2_pt, d2_tp


def surface_distances(predictions: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5,
                      backend: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """``(d2_pt, d2_tp)``, int32 (B, H, W) each: at every boundary pixel of the prediction
    (``p > threshold``) the squared distance to the nearest boundary pixel of the target (``t > 0``),
    -1 elsewhere, and the mirror image; EDT_NONE where the opposite boundary is empty. CUDA tensors:
    on their device, no host synchronisation. CPU tensors (and ``backend="host"``):
    ``extract_boundaries`` + ``distance_transform_sq_np``, CPU tensors; the two agree exactly."""
    if _use_device(backend, predictions, targets):
        return _surface_device(predictions, targets, threshold)
    d2_pt, d2_tp = _surface_host(predictions, targets, threshold)
    return torch.from_numpy(d2_pt), torch.from_numpy(d2_tp)


def _as_surface(a, b, threshold: float, backend: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(predictions, targets) -> their surface distances; a (d2_pt, d2_tp) pair passes through.
    Both come back as (B, H * W)."""
    _check_backend(backend)
    if b is None:
        if not isinstance(a, (tuple, list)) or len(a) != 2:
            raise ValueError("need predictions and targets, or the pair surface_distances returns")
        d2_pt, d2_tp = a
    else:
        d2_pt, d2_tp = surface_distances(a, b, threshold, backend)
    if d2_pt.dtype != torch.int32 or d2_tp.dtype != torch.int32 or d2_pt.dim() < 2 or d2_pt.shape != d2_tp.shape \
            or d2_pt.device != d2_tp.device:
        raise ValueError(f"need two int32 tables of one shape (..., H, W) on one device, got {d2_pt.dtype} "
                         f"{tuple(d2_pt.shape)} and {d2_tp.dtype} {tuple(d2_tp.shape)}")
    H, W = d2_pt.shape[-2:]
    return d2_pt.reshape(-1, H * W), d2_tp.reshape(-1, H * W)


def _percentile_d2(d2: torch.Tensor, percentile: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(n, d2_(k)) of a (B, npx) table: the number of boundary pixels and their k-th smallest squared
    distance, k = (percentile n + 99) // 100 (nearest rank), int64; the second is meaningless where
    n = 0. The -1 entries sort first, so rank k sits at npx - n + k - 1."""
    n = (d2 >= 0).sum(dim=1)
    k = (percentile * n + 99) // 100
    idx = (d2.shape[1] - n + k - 1).clamp(0, d2.shape[1] - 1)
    return n, torch.sort(d2, dim=1)[0].gather(1, idx[:, None])[:, 0].to(torch.int64)


def _sqrt_f64(x: torch.Tensor) -> torch.Tensor:
    """Correctly rounded float64 square root of a non-negative integer tensor on its device (the CPU
    kernel of torch.sqrt may be an ulp off, numpy's is not; the GPU one is correctly rounded)."""
    x = x.to(torch.float64)
    return x.sqrt() if x.is_cuda else torch.from_numpy(np.sqrt(x.numpy()))


def compute_hausdorff_percentile_batch(predictions, targets=None, percentile: int = 95, threshold: float = 0.5,
                                       backend: str = "auto") -> torch.Tensor:
    """Per-sample ``percentile``-th percentile Hausdorff distance of the boundaries (HD95 by default),
    float64 on the tables' device: per direction the nearest-rank percentile of the boundary pixels'
    distances to the other boundary, the larger of the two directions; the square root of an exact
    integer, and the Hausdorff distance at ``percentile=100``. inf when either boundary is empty.
    Takes (predictions, targets) or the pair ``surface_distances`` returns."""
    percentile = _check_percentile(percentile)
    d2_pt, d2_tp = _as_surface(predictions, targets, threshold, backend)
    n_p, k_p = _percentile_d2(d2_pt, percentile)
    n_t, k_t = _percentile_d2(d2_tp, percentile)
    h = _sqrt_f64(torch.maximum(k_p, k_t).clamp_min(0))  # (-1 where a boundary is empty: inf below)
    return torch.where((n_p == 0) | (n_t == 0), torch.full_like(h, float("inf")), h)


def compute_assd_batch(predictions, targets=None, threshold: float = 0.5, backend: str = "auto") -> torch.Tensor:
    """Per-sample average symmetric surface distance, float64 on the tables' device: the mean over
    the boundary pixels of both boundaries of the distance to the other boundary. inf when either
    boundary is empty. Takes (predictions, targets) or the pair ``surface_distances`` returns."""
    d2_pt, d2_tp = _as_surface(predictions, targets, threshold, backend)

    def total(d2):
        return _sqrt_f64(d2.clamp_min(0)).sum(dim=1), (d2 >= 0).sum(dim=1)  # the -1 entries add 0
    s_p, n_p = total(d2_pt)
    s_t, n_t = total(d2_tp)
    assd = (s_p + s_t) / (n_p + n_t).clamp_min(1).to(torch.float64)
    return torch.where((n_p == 0) | (n_t == 0), torch.full_like(assd, float("inf")), assd)


def compute_surface_dice_batch(predictions, targets=None, tolerance: int = 2, smooth: float = 1e-6,
                               threshold: float = 0.5, backend: str = "auto") -> torch.Tensor:
    """Per-sample surface Dice at ``tolerance`` pixels, float64 on the tables' device:
    (m_p + m_t + smooth) / (n_p + n_t + smooth) with n the boundary sizes and m the boundary pixels
    within ``tolerance`` of the other boundary. Takes (predictions, targets) or the pair
    ``surface_distances`` returns."""
    tol2 = _check_surface_tolerance(tolerance) ** 2
    d2_pt, d2_tp = _as_surface(predictions, targets, threshold, backend)
    n = (d2_pt >= 0).sum(dim=1) + (d2_tp >= 0).sum(dim=1)
    m = ((d2_pt >= 0) & (d2_pt <= tol2)).sum(dim=1) + ((d2_tp >= 0) & (d2_tp <= tol2)).sum(dim=1)
    return (m.to(torch.float64) + smooth) / (n.to(torch.float64) + smooth)


_probability_table_of_batch = probability_table  # evaluate_model has a parameter of that name
# the per-image arrays evaluate_model(probability_metrics=True) adds, in this order
PROBABILITY_METRIC_KEYS = ("auroc_scores", "average_precision_scores", "ece_scores", "brier_scores",
                           "best_threshold_dice_scores", "best_thresholds")
# the per-image arrays evaluate_model(physics_metrics=True) adds, in this order
PHYSICS_METRIC_KEYS = ("rd_residuals", "pf_energies", "interface_fractions")


def _check_refine(refine) -> None:
    from .pde import PDERefine
    if refine is not None and not isinstance(refine, PDERefine):
        raise TypeError(f"refine must be a pde.PDERefine or None, got {type(refine).__name__}")


def _check_physics(D: float, a: float, eps: float) -> None:
    if not (D >= 0 and 0 < a < 1 and eps > 0):
        raise ValueError(f"physics_D = {D}, physics_a = {a}, physics_eps = {eps}: D >= 0, 0 < a < 1 and eps > 0 "
                         "are needed")


@torch.no_grad()
def evaluate_model(model, dataloader, device, threshold: float = 0.5, boundary_metrics: bool = True,
                   boundary_backend: str = "auto", object_metrics: bool = False, connectivity: int = 8,
                   min_object_area: int = 0, object_backend: str = "auto", probability_metrics: bool = False,
                   calibration_bins: int = 16, probability_backend: str = "auto",
                   probability_table: Optional[ProbabilityTable] = None, tta: Optional[str] = None,
                   tta_tile: int = 512, tta_overlap: int = 64, refine=None, physics_metrics: bool = False,
                   physics_D: float = 1.0, physics_a: float = 0.5, physics_eps: float = 0.05,
                   surface_metrics: bool = False, surface_percentile: int = 95, surface_tolerance: int = 2,
                   surface_backend: str = "auto") -> Dict[str, np.ndarray]:
    """Per-image Dice / IoU (fused counters on the GPU) and boundary F1 / Hausdorff over a loader
    (src/evaluate.py:279-350). The boundary metrics of a CUDA batch come from one
    ``boundary_counts`` call and one device->host copy per batch (``boundary_backend``: "auto",
    "host" or "device", as ``compute_boundary_f1_batch``). ``object_metrics=True`` adds
    ``object_f1_scores`` (IoU > 0.5), ``aji_scores`` and ``object_count_errors`` (n_p - n_t) from
    one ``object_counts`` call and one device->host copy per batch. ``probability_metrics=True``
    adds ``auroc_scores``, ``average_precision_scores``, ``ece_scores`` (``calibration_bins`` bins),
    ``brier_scores``, ``best_threshold_dice_scores`` and ``best_thresholds`` from one
    ``probability_table`` call and one device->host copy per batch; a ``ProbabilityTable`` passed as
    ``probability_table`` is updated with every batch (the pooled curves of the loader).
    ``tta="flip"`` / ``"d4"``: the outputs are the test-time-augmented probabilities of a
    ``predict.Predictor`` (tiles of at most ``tta_tile`` with ``tta_overlap`` overlap, 4 or 8
    symmetries) instead of ``model(images)``; everything downstream is unchanged.
    ``refine`` (a ``pde.PDERefine``): every batch's probabilities (after the blend, with ``tta``)
    are evolved under the PDE (``pde.evolve``) before the threshold and before every metric family.
    ``physics_metrics=True`` adds ``rd_residuals`` (per-image mean squared reaction-diffusion
    residual, with ``physics_D`` and ``physics_a``), ``pf_energies`` (per-image mean phase-field
    energy density, ``physics_eps``) and ``interface_fractions`` (the share of pixels with
    0.1 < u < 0.9) from one ``pde.energies`` call and one device->host copy per batch.
    ``surface_metrics=True`` adds ``hausdorff_percentile_distances`` (``surface_percentile``: 95 is
    HD95; NaN where a boundary is empty, as ``hausdorff_distances``), ``assd_distances`` (likewise) and
    ``surface_dice_scores`` (at ``surface_tolerance`` pixels) from one ``surface_distances`` call
    (``surface_backend``) and one device->host copy per batch."""
    predictor = None
    _check_refine(refine)  # both refused before any GPU work
    if physics_metrics:
        _check_physics(physics_D, physics_a, physics_eps)
    if surface_metrics:
        surface_percentile = _check_percentile(surface_percentile)
        surface_tolerance = _check_surface_tolerance(surface_tolerance)
        _check_backend(surface_backend)
    if refine is not None or physics_metrics:
        from .pde import energies as _energies, evolve as _evolve
    if tta is not None:  # refused before any GPU work
        from .predict import Predictor
        if tta not in ("flip", "d4"):
            raise ValueError(f"tta must be None, 'flip' or 'd4', got {tta!r}")
        predictor = Predictor(model, tile=tta_tile, overlap=tta_overlap, tta=tta, threshold=threshold)
    if probability_metrics:  # refused before any GPU work
        calibration_bins = _check_calibration_bins(calibration_bins)
        if probability_backend not in ("auto", "host", "device"):
            raise ValueError(f"backend must be 'auto', 'host' or 'device', got {probability_backend!r}")
    model.eval()
    if object_metrics:
        _check_objects(connectivity, min_object_area)
    dice, iou, bf1, hd = [], [], [], []
    of1, aji, cerr = [], [], []
    prob = [[] for _ in range(6)]
    phys = [[] for _ in range(3)]
    surf = [[] for _ in range(3)]
    for images, masks in dataloader:
        images, masks = images.to(device, non_blocking=True), masks.to(device, non_blocking=True)
        outputs = model(images) if predictor is None else predictor.predict_batch(images)[0]
        if refine is not None:
            outputs = _evolve(outputs, refine)
        _, scores = sample_counts(outputs, masks, threshold)
        s = scores.cpu().numpy()
        dice.extend(s[:, 0].tolist())
        iou.extend(s[:, 1].tolist())
        if boundary_metrics and _use_device(boundary_backend, outputs, masks):
            counts = boundary_counts(outputs, masks, threshold, 2)
            both = torch.stack([_f1_from_counts(counts, 2, 1e-6).to(torch.float32).to(torch.float64),
                                _hausdorff_from_counts(counts)]).cpu().numpy()
            bf1.extend(both[0].tolist())
            hd.extend(np.where(np.isfinite(both[1]), both[1], np.nan).tolist())
        elif boundary_metrics:
            bf1.extend(compute_boundary_f1_batch(outputs, masks, threshold=threshold, tolerance=2,
                                                 backend="host").tolist())
            for i in range(outputs.shape[0]):
                h = compute_hausdorff_distance(outputs[i:i + 1], masks[i:i + 1], threshold=threshold,
                                               backend="host")
                hd.append(h if np.isfinite(h) else np.nan)
        if object_metrics:
            counts = object_counts(outputs, masks, threshold, connectivity, min_object_area, object_backend)
            three = torch.stack([_object_f1_from_counts(counts, 0.5), _aji_from_counts(counts),
                                 (counts[:, OBJ_NP] - counts[:, OBJ_NT]).to(torch.float64)]).cpu().numpy()
            of1.extend(three[0].tolist())
            aji.extend(three[1].tolist())
            cerr.extend(three[2].tolist())
        if probability_metrics:
            table, extra = _probability_table_of_batch(outputs, masks, probability_backend)
            if probability_table is not None:
                probability_table.update(table, extra)
            thr, thr_dice = best_threshold_batch(table)
            six = torch.stack([compute_auroc_batch(table), compute_average_precision_batch(table),
                               compute_ece_batch(table, n_bins=calibration_bins), compute_brier_batch((table, extra)),
                               thr_dice, thr]).cpu().numpy()
            for acc, row in zip(prob, six):
                acc.extend(row.tolist())
        if physics_metrics:
            e, n = _energies(outputs, physics_D, physics_a, physics_eps)
            px = float(outputs.shape[-2] * outputs.shape[-1])
            three = torch.stack([e[:, 0], e[:, 1], n.to(torch.float64) / px]).cpu().numpy()
            for acc, row in zip(phys, three):
                acc.extend(row.tolist())
        if surface_metrics:
            pair = surface_distances(outputs, masks, threshold, surface_backend)
            three = torch.stack([compute_hausdorff_percentile_batch(pair, percentile=surface_percentile),
                                 compute_assd_batch(pair),
                                 compute_surface_dice_batch(pair, tolerance=surface_tolerance)]).cpu().numpy()
            three[:2] = np.where(np.isfinite(three[:2]), three[:2], np.nan)
            for acc, row in zip(surf, three):
                acc.extend(row.tolist())
    out = {"dice_scores": np.array(dice), "iou_scores": np.array(iou)}
    if boundary_metrics:
        out["boundary_f1_scores"] = np.array(bf1)
        out["hausdorff_distances"] = np.array(hd)
    if object_metrics:
        out["object_f1_scores"] = np.array(of1)
        out["aji_scores"] = np.array(aji)
        out["object_count_errors"] = np.array(cerr)
    if probability_metrics:
        for key, acc in zip(PROBABILITY_METRIC_KEYS, prob):
            out[key] = np.array(acc, dtype=np.float64)
    if physics_metrics:
        for key, acc in zip(PHYSICS_METRIC_KEYS, phys):
            out[key] = np.array(acc, dtype=np.float64)
    if surface_metrics:
        for key, acc in zip(SURFACE_METRIC_KEYS, surf):
            out[key] = np.array(acc, dtype=np.float64)
    return out


# ----------------------------------------------------------------------------
# Statistics and test-set evaluation (src/evaluate.py:349-523) — host-side, after training
# ----------------------------------------------------------------------------

def compute_statistics(metric_array: np.ndarray) -> Dict[str, float]:
    """Mean, sample std (ddof=1) and count over the non-NaN entries (src/evaluate.py:349-369)."""
    a = np.asarray(metric_array, dtype=np.float64)
    a = a[~np.isnan(a)]
    if a.size == 0:
        return {"mean": np.nan, "std": np.nan, "count": 0}
    return {"mean": float(a.mean()), "std": float(a.std(ddof=1)), "count": int(a.size)}


_NO_TEST = {"t_statistic": np.nan, "t_pvalue": np.nan, "wilcoxon_statistic": np.nan,
            "wilcoxon_pvalue": np.nan, "significant": False}


def compare_models_statistically(metrics_baseline: Dict[str, np.ndarray], metrics_pde: Dict[str, np.ndarray],
                                 alpha: float = 0.05) -> Dict[str, Dict[str, float]]:
    """Paired t-test + two-sided Wilcoxon signed-rank per metric over the images where both
    models have a value; significant if either p < alpha (src/evaluate.py:372-438)."""
    from scipy import stats
    out = {}
    for name, base in metrics_baseline.items():
        b = np.asarray(base, dtype=np.float64)
        p = np.asarray(metrics_pde[name], dtype=np.float64)
        keep = ~(np.isnan(b) | np.isnan(p))
        b, p = b[keep], p[keep]
        if b.size < 2:
            out[name] = dict(_NO_TEST)
            continue
        t_stat, t_p = stats.ttest_rel(b, p)
        w_stat, w_p = stats.wilcoxon(b, p, alternative="two-sided")
        sb, sp = compute_statistics(b), compute_statistics(p)
        out[name] = {"t_statistic": float(t_stat), "t_pvalue": float(t_p), "wilcoxon_statistic": float(w_stat),
                     "wilcoxon_pvalue": float(w_p), "significant": bool(t_p < alpha or w_p < alpha),
                     "baseline_mean": sb["mean"], "baseline_std": sb["std"], "pde_mean": sp["mean"],
                     "pde_std": sp["std"], "improvement": float(p.mean() - b.mean())}
    return out


def format_metric_report(metrics: Dict[str, np.ndarray], model_name: str = "Model") -> str:
    """'<Metric Title>: mean ± std (n=count)' lines (src/evaluate.py:441-472)."""
    lines = [f"\n{model_name} Performance:", "=" * 60]
    for name, arr in metrics.items():
        st = compute_statistics(arr)
        title = name.replace("_", " ").title()
        lines.append(f"{title}: {st['mean']:.4f} ± {st['std']:.4f} (n={st['count']})" if st["count"] > 0
                     else f"{title}: N/A")
    return "\n".join(lines)


def evaluate_on_test_set(model, test_dir, test_json, device, batch_size: int = 8, threshold: float = 0.5,
                         model_name: str = "Model", device_cache: bool = False, object_metrics: bool = False,
                         connectivity: int = 8, min_object_area: int = 0, probability_metrics: bool = False,
                         calibration_bins: int = 16,
                         probability_table: Optional[ProbabilityTable] = None, tta: Optional[str] = None,
                         tta_tile: int = 512, tta_overlap: int = 64, refine=None, physics_metrics: bool = False,
                         physics_D: float = 1.0, physics_a: float = 0.5, physics_eps: float = 0.05,
                         surface_metrics: bool = False, surface_percentile: int = 95, surface_tolerance: int = 2
                         ) -> Dict[str, np.ndarray]:
    """Per-image metrics of ``model`` on a COCO-annotated test folder (src/evaluate.py:476-522).
    ``device_cache=True`` serves the (bit-identical) batches from a device-resident cache
    (``dataset.DeviceCachedLoader``) instead of ``DataLoader`` workers; a set that does not fit
    falls back to them. ``object_metrics=True`` adds the object-level arrays of ``evaluate_model``,
    ``probability_metrics=True`` its probability-level arrays (ECE over ``calibration_bins`` bins;
    a ``ProbabilityTable`` passed as ``probability_table`` receives the pooled table of the set).
    ``tta``, ``tta_tile``, ``tta_overlap``: test-time augmentation, as ``evaluate_model``.
    ``refine``, ``physics_metrics``, ``physics_D``, ``physics_a``, ``physics_eps``: PDE refinement
    of the probabilities and the per-image physics arrays, as ``evaluate_model``.
    ``surface_metrics``, ``surface_percentile``, ``surface_tolerance``: the percentile Hausdorff
    distance, ASSD and surface Dice arrays, as ``evaluate_model``."""
    if probability_metrics:
        _check_calibration_bins(calibration_bins)
    _check_refine(refine)
    tta_kw = {} if tta is None else dict(tta=tta, tta_tile=tta_tile, tta_overlap=tta_overlap)
    if refine is not None:
        tta_kw["refine"] = refine
    if physics_metrics:
        _check_physics(physics_D, physics_a, physics_eps)
        tta_kw.update(physics_metrics=True, physics_D=physics_D, physics_a=physics_a, physics_eps=physics_eps)
    if surface_metrics:
        tta_kw.update(surface_metrics=True, surface_percentile=_check_percentile(surface_percentile),
                      surface_tolerance=_check_surface_tolerance(surface_tolerance))
    from torch.utils.data import DataLoader

    from .dataset import CellSegmentationDataset, DeviceCachedLoader
    print(f"\nEvaluating {model_name} on test set...")
    print("=" * 70)
    ds = CellSegmentationDataset(test_dir, test_json)
    loader = None
    if device_cache:
        try:
            loader = DeviceCachedLoader(ds, batch_size, shuffle=False, device=device)
        except ValueError as e:
            if "max_bytes" not in str(e):
                raise
            print(f"device cache not used, falling back to DataLoader workers: {e}")
    if loader is None:
        loader = DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=2,
                            pin_memory=torch.cuda.is_available())
    print(f"Test samples: {len(ds)}")
    metrics = evaluate_model(model, loader, device, threshold=threshold, object_metrics=object_metrics,
                             connectivity=connectivity, min_object_area=min_object_area,
                             probability_metrics=probability_metrics, calibration_bins=calibration_bins,
                             probability_table=probability_table, **tta_kw)
    print(format_metric_report(metrics, model_name=model_name))
    return metrics


__all__ = ["compute_iou", "compute_iou_batch", "extract_boundaries", "compute_boundary_f1",
           "compute_boundary_f1_batch", "compute_hausdorff_distance", "boundary_counts",
           "extract_boundaries_device", "compute_hausdorff_distance_batch", "evaluate_model",
           "compute_dice_score_batch", "compute_statistics", "compare_models_statistically",
           "format_metric_report", "evaluate_on_test_set", "object_counts", "label_components",
           "compute_object_f1_batch", "compute_aji_batch", "probability_table", "threshold_sweep_counts",
           "compute_auroc_batch", "compute_average_precision_batch", "compute_ece_batch", "compute_brier_batch",
           "best_threshold_batch", "ProbabilityTable", "PHYSICS_METRIC_KEYS", "EDT_NONE", "SURFACE_METRIC_KEYS",
           "distance_transform_sq_np", "distance_transform_sq", "surface_distances",
           "compute_hausdorff_percentile_batch", "compute_assd_batch", "compute_surface_dice_batch"]
