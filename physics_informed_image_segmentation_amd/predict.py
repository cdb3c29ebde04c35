"""Whole-image inference: tiled, test-time-augmented prediction on the GPU.

An image of any size is cut into overlapping tiles (reflected past its edges), each tile is
optionally presented under the symmetries of the grid, the U-Net runs on chunks of tiles, and the
tile probabilities are blended back into one map. The data movement around the forwards is two
launches (csrc/infer.hip: ``pis_tile_gather`` per chunk, ``pis_tile_blend`` once); their definition
is include/pis_capi.h's, restated here in float32 numpy with the same operation order
(``tile_plan``, ``gather_tiles_np``, ``blend_tiles_np``): the definition of record, in the role of
``PackedSamples.warp``. The kernels agree with it bit for bit (tests/test_predict_gpu.py).

``clean_mask`` drops specks and fills holes of a predicted mask on the existing component
labelling (``label_components``); its host path is scipy.ndimage and is the oracle.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip

TTA_MASKS = {None: 0x01, "none": 0x01, "flip": 0x0F, "d4": 0xFF}
TILE_MIN, TILE_MAX, OVERLAP_MAX, SIDE_MAX = 16, 2048, 256, 32768


# ----------------------------------------------------------------------------
# The definition: tile origins, job numbering, gather and blend in numpy
# ----------------------------------------------------------------------------

def ceil16(n: int) -> int:
    return (int(n) + 15) // 16 * 16


def tile_count(n: int, t: int, o: int) -> int:
    """K(n, t, o): tiles along an axis of length n with tile t and overlap o."""
    return 1 if n <= t else -(-(n - o) // (t - o))


def tile_origins(n: int, t: int, o: int) -> List[int]:
    """origin(k) = min(k (t - o), max(n - t, 0)): the last tile is pulled back to end at the edge."""
    return [min(k * (t - o), max(n - t, 0)) for k in range(tile_count(n, t, o))]


def ramp_weights(t: int, o: int) -> np.ndarray:
    """w1(l, t, o) = min(l + 1, t - l, o) for o >= 1, 1 for o == 0, as int64 (t,)."""
    l = np.arange(t, dtype=np.int64)
    return np.minimum(np.minimum(l + 1, t - l), o) if o >= 1 else np.ones(t, np.int64)


def reflect_index(i, n: int) -> np.ndarray:
    """reflect(i, n) of include/pis_capi.h: 0 if n == 1, else m = i mod (2n - 2), m < n ? m : 2n - 2 - m."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def _check_geometry(H: int, W: int, th: int, tw: int, ov: int, sym_mask: int) -> None:
    for t in (th, tw):
        if not (TILE_MIN <= t <= TILE_MAX and t % 16 == 0):
            raise ValueError(f"tile {th} x {tw}: multiples of 16 in [{TILE_MIN}, {TILE_MAX}] are needed")
    if not 0 <= ov <= min(th, tw) // 2 or ov > OVERLAP_MAX:
        raise ValueError(f"overlap {ov}: 0 <= overlap <= min(th, tw) / 2 = {min(th, tw) // 2} and <= {OVERLAP_MAX} "
                         "is needed")
    if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
        raise ValueError(f"image {H} x {W}: sides in [1, {SIDE_MAX}] are needed")
    if not 1 <= sym_mask <= 0xFF:
        raise ValueError(f"sym_mask {sym_mask:#x}: a non-empty set of the codes 0..7 is needed")
    if sym_mask & 0xF0 and th != tw:
        raise ValueError(f"a symmetry code >= 4 transposes: a square tile is needed, got {th} x {tw}")


class TilePlan(NamedTuple):
    """The tiling of one H x W image: tile size, overlap, the origins per axis and the symmetry codes in
    job order. Job ``j = ((s Ky + ky) Kx + kx) Ns + qi`` for source ``s``."""
    H: int
    W: int
    th: int
    tw: int
    ov: int
    oy: Tuple[int, ...]
    ox: Tuple[int, ...]
    sym_mask: int
    codes: Tuple[int, ...]

    @property
    def Ky(self) -> int:
        return len(self.oy)

    @property
    def Kx(self) -> int:
        return len(self.ox)

    @property
    def Ns(self) -> int:
        return len(self.codes)

    def jobs(self, S: int = 1) -> int:
        return S * self.Ky * self.Kx * self.Ns


def _sym_mask(tta) -> int:
    if isinstance(tta, (int, np.integer)) and not isinstance(tta, bool):
        return int(tta)
    try:
        return TTA_MASKS[tta]
    except (KeyError, TypeError):
        raise ValueError(f"tta must be None, 'none', 'flip', 'd4' or a symmetry mask, got {tta!r}") from None


def tile_plan(H: int, W: int, tile: Union[int, Sequence[int]] = 512, overlap: int = 64, tta=None) -> TilePlan:
    """The plan of an H x W image. ``tile`` an int: the tile is chosen for the image,
    ``th = min(tile, ceil16(H))``, ``tw`` likewise, both ``min(tile, ceil16(max(H, W)))`` when a
    symmetry transposes, the overlap is lowered to half the smaller tile side where the tile shrank
    below twice the overlap, and it is 0 where one tile holds the whole image (every weight is then
    1, and without symmetries the result is the network's output bit for bit). ``tile`` a pair
    ``(th, tw)``: tile and overlap are used as given. ``tta``: None / "none" (code 0), "flip"
    (codes 0..3), "d4" (all eight) or an 8-bit set of codes."""
    mask = _sym_mask(tta)
    H, W, ov = int(H), int(W), int(overlap)
    if isinstance(tile, (int, np.integer)):
        tile = int(tile)
        if not (TILE_MIN <= tile <= TILE_MAX and tile % 16 == 0):
            raise ValueError(f"tile {tile}: a multiple of 16 in [{TILE_MIN}, {TILE_MAX}] is needed")
        if not 0 <= ov <= min(tile // 2, OVERLAP_MAX):
            raise ValueError(f"overlap {ov}: 0 <= overlap <= tile / 2 = {tile // 2} and <= {OVERLAP_MAX} is needed")
        if mask & 0xF0:
            th = tw = min(tile, ceil16(max(H, W)))
        else:
            th, tw = min(tile, ceil16(H)), min(tile, ceil16(W))
        ov = min(ov, min(th, tw) // 2)
        if H <= th and W <= tw:  # one tile: no neighbour to ramp against, every weight is 1
            ov = 0
    else:
        th, tw = (int(v) for v in tile)
    _check_geometry(H, W, th, tw, ov, mask)
    return TilePlan(H, W, th, tw, ov, tuple(tile_origins(H, th, ov)), tuple(tile_origins(W, tw, ov)), mask,
                    tuple(q for q in range(8) if mask >> q & 1))


def apply_symmetry_np(t: np.ndarray, q: int) -> np.ndarray:
    """``dataset.apply_symmetry`` on the last two axes of a numpy array."""
    if q & 1:
        t = t[..., :, ::-1]
    if q & 2:
        t = t[..., ::-1, :]
    if q & 4:
        t = np.swapaxes(t, -1, -2)
    return t


def invert_symmetry_np(t: np.ndarray, q: int) -> np.ndarray:
    """The inverse of ``apply_symmetry_np(., q)``."""
    if q & 4:
        t = np.swapaxes(t, -1, -2)
    if q & 2:
        t = t[..., ::-1, :]
    if q & 1:
        t = t[..., :, ::-1]
    return t


def gather_tiles_np(src: np.ndarray, plan: TilePlan, norm: Optional[np.ndarray] = None, first_job: int = 0,
                    n_jobs: Optional[int] = None) -> np.ndarray:
    """``pis_tile_gather`` in numpy: ``src`` (S, H, W) float32, or uint8 with ``norm`` (S, 2) float32
    ``(lo, den)``; returns (n_jobs, 1, th, tw) float32 for the jobs [first_job, first_job + n_jobs)."""
    src = np.asarray(src)
    if src.ndim != 3 or src.shape[1:] != (plan.H, plan.W):
        raise ValueError(f"src {src.shape}: (S, {plan.H}, {plan.W}) is needed")
    if src.dtype == np.uint8:
        if norm is None:
            raise ValueError("uint8 sources need norm (S, 2)")
        norm = np.asarray(norm, np.float32).reshape(src.shape[0], 2)
    elif src.dtype != np.float32:
        raise TypeError(f"src must be uint8 or float32, got {src.dtype}")
    J = plan.jobs(src.shape[0])
    n_jobs = J - first_job if n_jobs is None else n_jobs
    if not (first_job >= 0 and n_jobs >= 1 and first_job + n_jobs <= J):
        raise ValueError(f"jobs [{first_job}, {first_job + n_jobs}) are not within [0, {J})")
    out = np.empty((n_jobs, 1, plan.th, plan.tw), np.float32)
    for j in range(first_job, first_job + n_jobs):
        t, qi = divmod(j, plan.Ns)
        t, kx = divmod(t, plan.Kx)
        s, ky = divmod(t, plan.Ky)
        rows = reflect_index(plan.oy[ky] + np.arange(plan.th), plan.H)
        cols = reflect_index(plan.ox[kx] + np.arange(plan.tw), plan.W)
        T = src[s][rows[:, None], cols[None, :]]
        if src.dtype == np.uint8:
            T = (T.astype(np.float32) - norm[s, 0]) / norm[s, 1]  # float32 throughout, each step rounded
        out[j - first_job, 0] = apply_symmetry_np(T, plan.codes[qi])
    return out


def blend_tiles_np(u: np.ndarray, plan: TilePlan, S: int = 1, threshold: float = 0.5
                   ) -> Tuple[np.ndarray, np.ndarray]:
    """``pis_tile_blend`` in numpy: ``u`` (J, 1, th, tw) float32 -> (prob (S, H, W) float32, mask
    (S, H, W) uint8). Tiles are visited in the order s, ky, kx, qi, so every pixel accumulates its
    covers in the kernel's order; each multiply, add and the division are float32 operations."""
    H, W, th, tw = plan.H, plan.W, plan.th, plan.tw
    u = np.asarray(u, np.float32).reshape(plan.jobs(S), th, tw)
    wy, wx = ramp_weights(th, plan.ov), ramp_weights(tw, plan.ov)
    acc = np.zeros((S, H, W), np.float32)
    wsum = np.zeros((S, H, W), np.int64)
    j = 0
    for s in range(S):
        for y0 in plan.oy:
            hh = min(th, H - y0)
            for x0 in plan.ox:
                ww = min(tw, W - x0)
                w = wy[:hh, None] * wx[None, :ww]
                wf = w.astype(np.float32)
                for q in plan.codes:
                    v = invert_symmetry_np(u[j], q)[:hh, :ww]
                    acc[s, y0:y0 + hh, x0:x0 + ww] = acc[s, y0:y0 + hh, x0:x0 + ww] + wf * v
                    wsum[s, y0:y0 + hh, x0:x0 + ww] += w
                    j += 1
    with np.errstate(invalid="ignore"):
        prob = acc / wsum.astype(np.float32)
        mask = (prob > np.float32(threshold)).astype(np.uint8)
    return prob, mask


# ----------------------------------------------------------------------------
# The two launches
# ----------------------------------------------------------------------------

def _aligned_sources(x: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(S, H, W) uint8 / float32 CUDA sources -> (a tensor whose samples start on 16-byte boundaries,
    the stride in bytes): the tensor itself where H * W already allows it, else one padded copy."""
    S, H, W = x.shape
    x = x.contiguous()
    row = H * W * x.element_size()
    if row % 16 == 0 and x.data_ptr() % 16 == 0:
        return x, row
    per = (row + 15) // 16 * 16 // x.element_size()
    buf = torch.empty((S, per), dtype=x.dtype, device=x.device)
    buf[:, :H * W] = x.reshape(S, H * W)
    return buf, per * x.element_size()


def gather_tiles(src: torch.Tensor, plan: TilePlan, norm: Optional[torch.Tensor] = None, first_job: int = 0,
                 n_jobs: Optional[int] = None) -> torch.Tensor:
    """One ``pis_tile_gather`` launch on the current stream: ``src`` (S, H, W) CUDA uint8 (with ``norm``
    (S, 2) float32 on the device) or float32 -> (n_jobs, 1, th, tw) float32."""
    _hip.require_cuda(src, "gather_tiles")
    if src.dim() != 3 or tuple(src.shape[1:]) != (plan.H, plan.W):
        raise ValueError(f"src {tuple(src.shape)}: (S, {plan.H}, {plan.W}) is needed")
    if src.dtype == torch.uint8:
        if norm is None:
            raise ValueError("uint8 sources need norm (S, 2)")
        norm = norm.to(device=src.device, dtype=torch.float32).contiguous()
        fmt = _hip.PIS_CACHE_IMG_U8
    elif src.dtype == torch.float32:
        fmt, norm = _hip.PIS_CACHE_IMG_F32, None
    else:
        raise TypeError(f"src must be uint8 or float32, got {src.dtype}")
    S = src.shape[0]
    n_jobs = plan.jobs(S) - first_job if n_jobs is None else n_jobs
    out = torch.empty((max(n_jobs, 0), 1, plan.th, plan.tw), dtype=torch.float32, device=src.device)
    buf, stride = _aligned_sources(src)
    with torch.cuda.device(src.device):
        _hip.call("pis_tile_gather", _hip.ptr(buf), fmt, stride, _hip.ptr(norm), S, plan.H, plan.W, plan.th, plan.tw,
                  plan.ov, plan.sym_mask, first_job, n_jobs, _hip.ptr(out), _hip.stream_handle(src.device))
    return out


def blend_tiles(u: torch.Tensor, plan: TilePlan, S: int = 1, threshold: float = 0.5, want_mask: bool = True
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """One ``pis_tile_blend`` launch on the current stream: ``u`` (J, 1, th, tw) float32 CUDA ->
    (prob (S, H, W) float32, mask (S, H, W) uint8 or None)."""
    _hip.require_cuda(u, "blend_tiles")
    if u.dtype != torch.float32 or u.numel() != plan.jobs(S) * plan.th * plan.tw:
        raise ValueError(f"u {tuple(u.shape)} {u.dtype}: ({plan.jobs(S)}, 1, {plan.th}, {plan.tw}) float32 is needed")
    u = u.contiguous()
    prob = torch.empty((S, plan.H, plan.W), dtype=torch.float32, device=u.device)
    mask = torch.empty((S, plan.H, plan.W), dtype=torch.uint8, device=u.device) if want_mask else None
    with torch.cuda.device(u.device):
        _hip.call("pis_tile_blend", _hip.ptr(u), S, plan.H, plan.W, plan.th, plan.tw, plan.ov, plan.sym_mask,
                  ctypes.c_float(float(threshold)), _hip.ptr(prob), _hip.ptr(mask), _hip.stream_handle(u.device))
    return prob, mask


def chunk_starts(J: int, batch_tiles: int) -> Tuple[int, List[int]]:
    """(chunk size, first job of every chunk): every chunk has the same size ``min(batch_tiles, J)``
    (the engine re-plans its buffers on a new batch size); the last one is pulled back to end at J
    and repeats jobs of the chunk before it, whose outputs are ignored."""
    n = min(batch_tiles, J)
    return n, [min(k * n, J - n) for k in range(-(-J // n))]


# ----------------------------------------------------------------------------
# Predictor
# ----------------------------------------------------------------------------

class Predictor:
    """Tiled, test-time-augmented prediction with a trained ``UNet`` (eval mode, no gradients).

    ``tile`` / ``overlap``: the largest tile and the overlap of neighbouring tiles (``tile_plan``
    chooses the tile per image). ``tta``: None, "flip" (4 symmetries) or "d4" (all 8). One
    ``pis_tile_gather`` and one forward per chunk of ``batch_tiles`` jobs, one ``pis_tile_blend``
    at the end; no call synchronises with the host. The tile outputs of all jobs are held in one
    buffer; a buffer above ``max_workspace_bytes`` (default 8 GiB: a choice, not a measurement) is
    refused before any GPU work. ``refine`` (a ``pde.PDERefine``): the blended whole-image
    probabilities are evolved under the PDE (``pde.evolve``, any H and W) and the mask returned is
    the one the evolve launch wrote, ``refined > threshold``."""

    def __init__(self, model, tile: int = 512, overlap: int = 64, tta: Optional[str] = None, batch_tiles: int = 8,
                 threshold: float = 0.5, max_workspace_bytes: int = 8 << 30, refine=None):
        if tta not in (None, "flip", "d4"):
            raise ValueError(f"tta must be None, 'flip' or 'd4', got {tta!r}")
        if int(batch_tiles) < 1:
            raise ValueError(f"batch_tiles must be >= 1, got {batch_tiles!r}")
        tile_plan(int(tile), int(tile), int(tile), int(overlap), tta)  # refuses a bad tile or overlap
        self.model = model
        self.tile, self.overlap, self.tta = int(tile), int(overlap), tta
        self.batch_tiles, self.threshold = int(batch_tiles), float(threshold)
        self.max_workspace_bytes = int(max_workspace_bytes)
        if refine is not None:
            from .pde import PDERefine
            if not isinstance(refine, PDERefine):
                raise TypeError(f"refine must be a pde.PDERefine or None, got {type(refine).__name__}")
        self.refine = refine

    def plan(self, H: int, W: int) -> TilePlan:
        return tile_plan(H, W, self.tile, self.overlap, self.tta)

    @torch.no_grad()
    def _run(self, src: torch.Tensor, norm: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        S, H, W = src.shape
        plan = self.plan(H, W)
        J = plan.jobs(S)
        need = J * plan.th * plan.tw * 4
        if need > self.max_workspace_bytes:
            raise ValueError(f"the tile outputs of {S} image(s) of {H} x {W} ({J} tiles of {plan.th} x {plan.tw}) "
                             f"need {need} bytes, above max_workspace_bytes = {self.max_workspace_bytes}: "
                             "predict fewer images per call, or use fewer symmetries or less overlap")
        self.model.eval()
        u = torch.empty((J, 1, plan.th, plan.tw), dtype=torch.float32, device=src.device)
        n, starts = chunk_starts(J, self.batch_tiles)
        buf, stride = _aligned_sources(src)
        fmt = _hip.PIS_CACHE_IMG_U8 if src.dtype == torch.uint8 else _hip.PIS_CACHE_IMG_F32
        tiles = torch.empty((n, 1, plan.th, plan.tw), dtype=torch.float32, device=src.device)
        done = 0
        with torch.cuda.device(src.device):
            st = _hip.stream_handle(src.device)
            for first in starts:
                _hip.call("pis_tile_gather", _hip.ptr(buf), fmt, stride, _hip.ptr(norm), S, H, W, plan.th, plan.tw,
                          plan.ov, plan.sym_mask, first, n, _hip.ptr(tiles), st)
                out = self.model(tiles)
                # the eval forward returns a tensor of its own (not an engine buffer); it is copied
                # into u before the next forward all the same, so that would not matter
                u[done:first + n].copy_(out[done - first:])
                done = first + n
        if self.refine is not None:
            from .pde import evolve
            prob, _ = blend_tiles(u, plan, S, self.threshold, want_mask=False)
            prob, mask = evolve(prob, self.refine, threshold=self.threshold)
        else:
            prob, mask = blend_tiles(u, plan, S, self.threshold)
        return prob.unsqueeze(1), mask.unsqueeze(1)

    def predict_batch(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``x`` (B, 1, H, W) float32 on the GPU, already normalised -> (prob (B, 1, H, W) float32,
        mask (B, 1, H, W) uint8 in {0, 1}) on the device."""
        _hip.require_cuda(x, "Predictor.predict_batch")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"expected input (B, 1, H, W), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError("Predictor expects float32 input")
        return self._run(x.detach()[:, 0], None)

    def predict_image(self, img: np.ndarray, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One (H, W) uint8 or float image under the dataset's whole-image min-max
        (``lo = min``, ``den = max - min + 1e-8`` in float32) -> (prob (H, W), mask (H, W)) on the
        device. A uint8 image is uploaded as uint8 and normalised by the gather."""
        img = np.asarray(img)
        if img.ndim != 2 or img.size == 0:
            raise ValueError(f"expected an (H, W) image, got shape {img.shape}")
        if device is None:
            device = next(self.model.parameters()).device
        device = torch.device(device)
        if device.type != "cuda":
            raise _hip.HipError(f"Predictor.predict_image: the model is on {device}; this build has no CPU fallback")
        if img.dtype == np.uint8:
            lo, hi = int(img.min()), int(img.max())
            norm = np.array([[np.float32(lo), np.float32(hi - lo) if hi > lo else np.float32(1e-8)]], np.float32)
            src = torch.from_numpy(np.array(img, order="C"))[None].to(device)  # a copy: PIL's arrays are read-only
            prob, mask = self._run(src, torch.from_numpy(norm).to(device))
        else:
            prob, mask = self._run(torch.from_numpy(normalise_image(img))[None].to(device), None)
        return prob[0, 0], mask[0, 0]


def normalise_image(img: np.ndarray) -> np.ndarray:
    """The dataset's whole-image min-max in float32: ``(img - min) / (max - min + 1e-8)``."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    return (img - img.min()) / (img.max() - img.min() + 1e-8)


# ----------------------------------------------------------------------------
# Mask clean-up
# ----------------------------------------------------------------------------

def _check_clean(min_area: int, connectivity: int, backend: str) -> None:
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if int(min_area) < 0:
        raise ValueError(f"min_area must be >= 0, got {min_area!r}")
    if backend not in ("auto", "host", "device"):
        raise ValueError(f"backend must be 'auto', 'host' or 'device', got {backend!r}")


def _clean_host(fg: np.ndarray, min_area: int, fill_holes: bool, connectivity: int) -> np.ndarray:
    from scipy import ndimage
    eight, four = np.ones((3, 3), bool), ndimage.generate_binary_structure(2, 1)
    out = np.empty(fg.shape, np.uint8)
    for i, m in enumerate(fg):
        if min_area > 1:
            lab, n = ndimage.label(m, structure=eight if connectivity == 8 else four)
            m = (np.bincount(lab.ravel(), minlength=n + 1) >= min_area)[lab] & (lab > 0)
        if fill_holes:  # the outside invades through the complementary connectivity
            m = ndimage.binary_fill_holes(m, structure=four if connectivity == 8 else eight)
        out[i] = m
    return out


def clean_mask(mask: torch.Tensor, min_area: int = 0, fill_holes: bool = False, connectivity: int = 8,
               backend: str = "auto") -> torch.Tensor:
    """Clean a binary mask ((H, W), (B, H, W) or (B, 1, H, W); foreground: > 0): objects (connected
    components under ``connectivity``) below ``min_area`` pixels are dropped, then, with
    ``fill_holes``, every hole is filled. A hole is a background component that does not touch the
    frame, under the complementary connectivity: 4 for 8-connected foreground, 8 for 4-connected.
    Returns uint8 in {0, 1} of the input's shape, on its device. CUDA masks: two
    ``label_components`` calls and a few elementwise steps, no host synchronisation; CPU masks
    (and ``backend="host"``): scipy.ndimage, the oracle. The two agree exactly."""
    from .evaluate import _bhw, _use_device, label_components
    _check_clean(min_area, connectivity, backend)
    min_area = int(min_area)
    m = _bhw(mask)
    if not _use_device(backend, m, m):
        out = _clean_host(m.cpu().numpy() > 0, min_area, bool(fill_holes), connectivity)
        return torch.from_numpy(out).to(mask.device).reshape(mask.shape)
    B, H, W = m.shape
    if min_area > 1:
        fg = label_components(m, 0.0, connectivity, min_area, backend="device")[0] > 0
    else:
        fg = m > 0
    if fill_holes:
        lab = label_components((~fg).to(torch.float32), 0.0, 4 if connectivity == 8 else 8, 0,
                               backend="device")[0].to(torch.int64)
        # the background components that reach the frame
        frame = torch.cat([lab[:, 0, :], lab[:, -1, :], lab[:, :, 0], lab[:, :, -1]], dim=1)
        outside = torch.zeros((B, H * W + 1), dtype=torch.bool, device=m.device)
        outside.scatter_(1, frame, True)
        outside[:, 0] = True  # label 0: the foreground
        fg = fg | ~outside.gather(1, lab.reshape(B, H * W)).reshape(B, H, W)
    return fg.to(torch.uint8).reshape(mask.shape)


__all__ = ["Predictor", "clean_mask", "tile_plan", "TilePlan", "gather_tiles_np", "blend_tiles_np", "gather_tiles",
           "blend_tiles", "tile_origins", "tile_count", "reflect_index", "ramp_weights", "chunk_starts",
           "normalise_image"]
