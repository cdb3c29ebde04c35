"""Data feeding the step (src/dataset.py:9-118).

``CellSegmentationDataset`` restates the reference loader's behaviour (COCO
polygons filled with PIL, NEAREST mask resize, bilinear image resize,
per-image min-max) — host-side, outside the kernel path.
``SyntheticDiscDataset`` is the benchmark/parity generator of SURVEY.md
§8(c)-(d): per-sample union of random discs, noisy image, min-max;
``DeviceDiscLoader`` rasterises the same samples on the GPU (§8(f) row 1).
``DeviceCachedLoader`` keeps any dataset, preprocessed once on the host
(``pack_samples``), resident on the GPU and assembles every batch there
(``pis_cache_batch``, csrc/cache.hip), optionally under a random affine and intensity
augmentation per sample and epoch (``AffineAugment``, ``pis_cache_batch_affine``).
"""
from __future__ import annotations

import json
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import torch
from torch.utils.data import Dataset, Subset


class CellSegmentationDataset(Dataset):
    def __init__(self, image_dir, annotation_file, image_size=(128, 128), transform=None):
        self.image_dir = Path(image_dir).resolve()
        self.image_size = tuple(image_size)
        self.transform = transform
        with open(Path(annotation_file).resolve(), "r") as f:
            coco = json.load(f)
        self.images_dict = {img["id"]: img for img in coco["images"]}
        self.anns_by_image = {}
        for ann in coco["annotations"]:
            self.anns_by_image.setdefault(ann["image_id"], []).append(ann)
        self.image_ids, missing = [], []
        for img_id, info in self.images_dict.items():
            if img_id not in self.anns_by_image:
                continue
            if (self.image_dir / info["file_name"]).exists():
                self.image_ids.append(img_id)
            else:
                missing.append(info["file_name"])
        if missing:
            print(f"Warning: {len(missing)} image(s) referenced in annotations but not found on disk:")
            for name in missing[:10]:
                print(f"  - {name}")
            if len(missing) > 10:
                print(f"  ... and {len(missing) - 10} more")
            print(f"These images will be skipped. Dataset size: {len(self.image_ids)}")

    def __len__(self):
        return len(self.image_ids)

    def _mask(self, anns, hw, size):
        from PIL import Image, ImageDraw
        H, W = hw
        canvas = Image.new("L", (W, H), 0)
        draw = ImageDraw.Draw(canvas)
        for ann in anns:
            seg = ann.get("segmentation", [])
            if isinstance(seg, list):
                for poly in seg:
                    if len(poly) >= 6:
                        draw.polygon(np.asarray(poly).reshape(-1, 2).flatten().tolist(), outline=1, fill=1)
        canvas = canvas.resize(size, resample=Image.NEAREST)
        return (np.asarray(canvas, dtype=np.float32) > 0).astype(np.float32)

    def raw_item(self, idx):
        """``(image_u8, mask_u8)``: the resized grey image as PIL returns it, (H, W) uint8, before
        the min-max normalisation, and the binary mask as uint8 — what ``__getitem__`` is computed
        from, and what the device cache stores (``pack_samples``). No ``transform`` is applied."""
        from PIL import Image
        image_id = self.image_ids[idx]
        info = self.images_dict[image_id]
        img = Image.open(self.image_dir / info["file_name"]).convert("L")
        img = np.asarray(img.resize(self.image_size, resample=Image.BILINEAR), dtype=np.uint8)
        mask = self._mask(self.anns_by_image[image_id], (info["height"], info["width"]), self.image_size)
        return img, mask.astype(np.uint8)

    def __getitem__(self, idx):
        img, mask = self.raw_item(idx)
        img, mask = img.astype(np.float32), mask.astype(np.float32)
        img = (img - img.min()) / (img.max() - img.min() + 1e-8)
        image = torch.from_numpy(img).unsqueeze(0)
        mask_t = torch.from_numpy(mask).unsqueeze(0)
        if self.transform is not None:
            image, mask_t = self.transform(image), self.transform(mask_t)
        return image, mask_t


def disc_params(H: int, W: int, g: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The disc centres and radii of one sample, drawn in the generator's order."""
    n = int(torch.randint(5, 15, (1,), generator=g))
    cx = torch.rand(n, generator=g) * W
    cy = torch.rand(n, generator=g) * H
    rad = (0.03 + 0.07 * torch.rand(n, generator=g)) * min(H, W)
    return cx, cy, rad


def disc_sample(H: int, W: int, g: torch.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """One (image, mask) pair of the SURVEY.md §8(c) generator."""
    rows, cols = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cx, cy, rad = disc_params(H, W, g)
    inside = torch.zeros(H, W, dtype=torch.bool)
    for k in range(cx.numel()):
        inside |= (cols - cx[k]) ** 2 + (rows - cy[k]) ** 2 <= rad[k] ** 2
    mask = inside.float()[None]
    img = 0.2 + 0.6 * mask + 0.1 * torch.randn(1, H, W, generator=g)
    img = (img - img.min()) / (img.max() - img.min() + 1e-8)
    return img, mask


def _sample_generator(seed: int, idx: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed * 1_000_003 + idx)


def shard_indices(ids, shuffle: bool, seed: int, epoch: int, rank: int, world: int):
    """This rank's sample ids for one epoch, as ``DistributedSampler(seed=seed)`` after
    ``set_epoch(epoch)``: a ``torch.randperm`` seeded ``seed + epoch`` when ``shuffle``, padded to
    a multiple of ``world`` by repeating its head, rank ``r`` taking every ``world``-th entry from
    ``r``. Shared by ``DeviceDiscLoader`` and ``DeviceCachedLoader``."""
    m = len(ids)
    perm = (torch.randperm(m, generator=torch.Generator().manual_seed(seed + epoch)).tolist()
            if shuffle else list(range(m)))
    idx = [ids[k] for k in perm]
    total = -(-m // world) * world
    idx += idx[:total - len(idx)]
    return idx[rank:total:world]


def _num_batches(m: int, batch_size: int, drop_last: bool) -> int:
    return m // batch_size if drop_last else -(-m // batch_size)


class DeviceDiscLoader:
    """Batches of the disc generator rasterised ON THE GPU (``pis_synth_discs``,
    SURVEY §8(f) row 1): only the disc parameters (<= 14 x 3 floats per sample) cross
    PCIe. Sample ``i`` uses the same generator as ``SyntheticDiscDataset`` item ``i``, so
    its mask is bit-identical to the host generator's; the image noise comes from a device
    hash of (seed, i, pixel) instead of torch.randn.

    Sharding follows ``DistributedSampler``: per epoch (``set_epoch``) a seeded
    permutation when ``shuffle``, padded to a multiple of ``world`` by repeating its head,
    rank ``r`` taking every ``world``-th index from ``r``. Iterating yields
    ``(images, masks)`` of shape (b, 1, H, W) on ``device``, already resident."""

    MAX_DISCS = 16

    def __init__(self, n: int, batch_size: int, image_size=(512, 512), seed: int = 42, shuffle: bool = True,
                 rank: int = 0, world: int = 1, device=None, drop_last: bool = False, subset=None):
        from . import _hip  # noqa: F401  (fail early when the library is missing)
        self.n, self.batch_size, self.size, self.seed = n, batch_size, tuple(image_size), seed
        self.shuffle, self.rank, self.world, self.drop_last = shuffle, rank, world, drop_last
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.epoch = 0
        self.dataset = SyntheticDiscDataset(n, image_size, seed)  # host twin (parity, len())
        self.ids = [int(i) for i in subset] if subset is not None else list(range(n))  # e.g. a train_fraction
        self._params = {}

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def indices(self):
        return shard_indices(self.ids, self.shuffle, self.seed, self.epoch, self.rank, self.world)

    def __len__(self):
        return _num_batches(len(self.indices()), self.batch_size, self.drop_last)

    def _disc(self, i: int):
        p = self._params.get(i)
        if p is None:
            H, W = self.size
            cx, cy, rad = disc_params(H, W, _sample_generator(self.seed, i))
            p = torch.stack([cx, cy, rad], 1)
            self._params[i] = p
        return p

    def batch(self, ids):
        from . import _hip
        H, W = self.size
        b = len(ids)
        discs = torch.zeros(b, self.MAX_DISCS, 3)
        nd = torch.empty(b, dtype=torch.int32)
        for j, i in enumerate(ids):
            p = self._disc(i)
            discs[j, :p.shape[0]] = p
            nd[j] = p.shape[0]
        dev = self.device
        discs_d = discs.to(dev, non_blocking=True)
        nd_d = nd.to(dev, non_blocking=True)
        sid = torch.tensor(ids, dtype=torch.int64).to(dev, non_blocking=True)
        img = torch.empty(b, 1, H, W, device=dev)
        mask = torch.empty(b, 1, H, W, device=dev)
        nws = _hip.lib().pis_synth_ws(b, H, W)
        ws = torch.empty((nws + 3) // 4, device=dev)
        _hip.call("pis_synth_discs", discs_d.data_ptr(), nd_d.data_ptr(), self.MAX_DISCS, self.seed, sid.data_ptr(),
                  img.data_ptr(), mask.data_ptr(), b, H, W, ws.data_ptr(), nws, _hip.stream_handle())
        return img, mask

    def __iter__(self):
        idx = self.indices()
        bs = self.batch_size
        stop = len(idx) - (len(idx) % bs if self.drop_last else 0)
        for k in range(0, stop, bs):
            yield self.batch(idx[k:k + bs])


class SyntheticDiscDataset(Dataset):
    """Deterministic synthetic cell-like masks: sample i is drawn from its own
    generator seeded ``seed * 1_000_003 + i`` (shard-independent)."""

    def __init__(self, n: int, image_size=(512, 512), seed: int = 42):
        self.n, self.size, self.seed = n, tuple(image_size), seed

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + idx)
        return disc_sample(self.size[0], self.size[1], g)


# ----------------------------------------------------------------------------
# device-resident dataset cache
# ----------------------------------------------------------------------------

def _pad16(nbytes: int) -> int:
    return -(-nbytes // 16) * 16


def _unwrap(dataset, indices=None):
    """The base dataset under any ``Subset`` wrappers and ``indices`` (default: all) mapped to it."""
    idx = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    while isinstance(dataset, Subset):
        sub = dataset.indices
        idx = [int(sub[i]) for i in idx]
        dataset = dataset.dataset
    return dataset, idx


def default_workers() -> int:
    """Host threads for packing: at most 16, whatever the machine's CPU count says."""
    return max(1, min(16, os.cpu_count() or 1))


class PackedSamples(NamedTuple):
    """Host arrays of a device cache (``pack_samples``). ``image`` and ``mask`` are (N, stride)
    uint8 views of the rows, each row padded to a multiple of 16 bytes.

    image_format "u8": H*W grey values per row, ``norm[i] = (lo, den)`` float32 with
    ``den = float(hi - lo)`` if ``hi > lo`` else ``1e-8`` — what ``img.max() - img.min() + 1e-8``
    rounds to in float32 — so ``(float(v) - lo) / den`` is the dataset item bit for bit;
    "f32": the float image of ``__getitem__`` verbatim, ``norm`` is None.
    mask_format "bits": ``np.packbits(mask, bitorder="little")``; "f32": verbatim."""
    image: np.ndarray
    mask: np.ndarray
    norm: Optional[np.ndarray]
    image_format: str
    mask_format: str
    size: Tuple[int, int]

    @property
    def nbytes(self) -> int:
        return self.image.nbytes + self.mask.nbytes + (self.norm.nbytes if self.norm is not None else 0)

    def __len__(self):
        return self.image.shape[0]

    def unpack(self, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Sample ``i`` as the (1, H, W) float32 pair the dataset returns (host reference of the kernel)."""
        H, W = self.size
        n = H * W
        if self.image_format == "u8":
            lo, den = self.norm[i]
            img = (self.image[i, :n].astype(np.float32) - lo) / den
        else:
            img = self.image[i, :4 * n].view(np.float32).copy()
        if self.mask_format == "bits":
            mask = np.unpackbits(self.mask[i], bitorder="little")[:n].astype(np.float32)
        else:
            mask = self.mask[i, :4 * n].view(np.float32).copy()
        return torch.from_numpy(img.reshape(1, H, W)), torch.from_numpy(mask.reshape(1, H, W))

    def warp(self, i: int, record) -> Tuple[torch.Tensor, torch.Tensor]:
        """Sample ``i`` under one affine record (``affine_record``: int32 ``a[6]``, float32 gain and
        bias), as the (1, H, W) float32 pair ``pis_cache_batch_affine`` writes. This is the
        DEFINITION of the augmentation (include/pis_capi.h restates it) and the kernel's oracle:
        int64 coordinates in 16.16 fixed point, float32 operations in the stated order, each
        rounded on its own, so the two agree bit for bit.

        For output pixel (y, x): ``SX = a0 x + a1 y + a2``, ``SY = a3 x + a4 y + a5``;
        ``x0 = SX >> 16``, ``fx = (SX >> 8) & 255`` (likewise y); the image is the bilinear mix of the
        four pixels at the reflected ``(y0 | y0 + 1, x0 | x0 + 1)`` with the 8-bit weights — for u8 an
        exact integer sum ``I < 2^24``, ``t = float(I) * 2^-16``, ``(t - lo) / den``; for f32
        ``((w00 v00 + w01 v01) + (w10 v10 + w11 v11)) * 2^-16`` — then ``gain * img + bias`` without
        a clamp; the mask is the nearest value, at ``reflect((S + 32768) >> 16)``."""
        H, W = self.size
        n = H * W
        rec = np.ascontiguousarray(record).view(np.int32).reshape(8)
        a = rec[:6].astype(np.int64)
        gain, bias = rec[6:].view(np.float32)
        y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
        SX = a[0] * x + a[1] * y + a[2]
        SY = a[3] * x + a[4] * y + a[5]
        x0, y0 = SX >> 16, SY >> 16
        fx, fy = (SX >> 8) & 255, (SY >> 8) & 255
        c0, c1 = reflect_index(x0, W), reflect_index(x0 + 1, W)
        r0, r1 = reflect_index(y0, H), reflect_index(y0 + 1, H)
        if self.image_format == "u8":
            v = self.image[i, :n].reshape(H, W).astype(np.int64)
            I = (256 - fy) * ((256 - fx) * v[r0, c0] + fx * v[r0, c1]) + fy * ((256 - fx) * v[r1, c0] + fx * v[r1, c1])
            lo, den = self.norm[i]
            img = (I.astype(np.float32) * np.float32(2.0 ** -16) - lo) / den
        else:
            v = self.image[i, :4 * n].view(np.float32).reshape(H, W)
            f32 = lambda w: w.astype(np.float32)
            top = f32((256 - fy) * (256 - fx)) * v[r0, c0] + f32((256 - fy) * fx) * v[r0, c1]
            bot = f32(fy * (256 - fx)) * v[r1, c0] + f32(fy * fx) * v[r1, c1]
            img = (top + bot) * np.float32(2.0 ** -16)
        img = gain * img + bias
        q = reflect_index((SY + 32768) >> 16, H) * W + reflect_index((SX + 32768) >> 16, W)
        if self.mask_format == "bits":
            mask = np.unpackbits(self.mask[i], bitorder="little")[:n].astype(np.float32)[q]
        else:
            mask = self.mask[i, :4 * n].view(np.float32)[q]
        assert img.dtype == np.float32 and mask.dtype == np.float32
        return (torch.from_numpy(np.ascontiguousarray(img).reshape(1, H, W)),
                torch.from_numpy(np.ascontiguousarray(mask).reshape(1, H, W)))


def reflect_index(i, n: int):
    """Index (array) ``i`` reflected into [0, n) about the edge pixels, which are not repeated (the
    loss stencils' boundary rule, ``np.pad(mode="reflect")``), any number of periods outside."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


# one record of pis_cache_batch_affine: int32 a[6], float gain, float bias
AFFINE_RECORD = np.dtype([("a", np.int32, 6), ("gain", np.float32), ("bias", np.float32)])
AFFINE_MAX_SIZE = 4096  # pis_cache_batch_affine: keeps the source coordinates' integer parts in 32 bits


def affine_record(size, rotate=0.0, scale=1.0, shift=(0.0, 0.0), flip=False, gain=1.0, bias=0.0) -> np.ndarray:
    """Records (``AFFINE_RECORD``) of the forward map ``p_out = c + s R(theta) F (p_in - c) + shift`` on
    an (H, W) = ``size`` grid: ``c = ((W - 1) / 2, (H - 1) / 2)``, points are (x, y), ``R`` turns x
    towards y by ``rotate`` degrees, ``F`` flips x when ``flip``, ``shift`` = (dx, dy) in pixels. Every
    argument may be an array of N values (``shift``: (N, 2)). A record holds the INVERSE map — the
    kernel goes from output pixels to source coordinates — computed in float64, times 65536,
    rounded with ``np.rint``; a coefficient that does not fit int32 raises ``ValueError``."""
    H, W = size
    th = np.deg2rad(np.asarray(rotate, np.float64))
    s = np.asarray(scale, np.float64)
    sh = np.asarray(shift, np.float64)
    f = np.where(np.asarray(flip, bool), -1.0, 1.0)
    th, s, f, dx, dy, gain, bias = np.broadcast_arrays(th, s, f, sh[..., 0], sh[..., 1], np.asarray(gain, np.float64),
                                                       np.asarray(bias, np.float64))
    cos, sin = np.cos(th), np.sin(th)
    # (s R F)^-1 = F R(-theta) / s
    m = np.stack([f * cos / s, f * sin / s, -sin / s, cos / s], -1)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    ox, oy = cx + dx, cy + dy  # where the centre lands
    off = np.stack([cx - (m[..., 0] * ox + m[..., 1] * oy), cy - (m[..., 2] * ox + m[..., 3] * oy)], -1)
    a = np.rint(np.stack([m[..., 0], m[..., 1], off[..., 0], m[..., 2], m[..., 3], off[..., 1]], -1) * 65536.0) + 0.0
    if not np.all(np.abs(a) < 2.0 ** 31):
        raise ValueError("affine_record: a coefficient does not fit the 16.16 int32 record "
                         f"(largest magnitude {np.abs(a).max() / 65536.0:g} pixels)")
    rec = np.zeros(a.shape[:-1], AFFINE_RECORD)
    rec["a"] = a.astype(np.int32)
    rec["gain"] = gain + 0.0  # + 0.0: no negative zero, the identity record has one bit pattern
    rec["bias"] = bias + 0.0
    return rec


@dataclass(frozen=True)
class AffineAugment:
    """Ranges of ``DeviceCachedLoader(augment=...)``'s random affine and intensity augmentation; each
    sample draws anew every epoch (``DeviceCachedLoader.affine_params``):

    rotate     uniform in +-``rotate`` degrees about the image centre
    scale      log-uniform in [1 / ``scale``, ``scale``]
    translate  uniform in +-``translate`` x (W, H)
    flip       a W flip with probability 1/2 (with the rotation: every reflection)
    gain       image x (1 +- ``gain``)
    bias       image + (+-``bias``), no clamp

    What falls outside the sample is its reflection. The defaults are a choice, not a measurement:
    the full circle because cells have no canonical orientation, the rest mild; no training run has
    tuned them."""
    rotate: float = 180.0
    scale: float = 1.25
    translate: float = 0.1
    flip: bool = True
    gain: float = 0.1
    bias: float = 0.05

    def __post_init__(self):
        if not (self.scale > 0 and self.rotate >= 0 and self.translate >= 0 and self.gain >= 0 and self.bias >= 0):
            raise ValueError(f"AffineAugment: scale must be positive and the other ranges non-negative, got {self}")


def _rows(rows, row_bytes: int) -> np.ndarray:
    out = np.zeros((len(rows), _pad16(row_bytes)), np.uint8)
    for k, r in enumerate(rows):
        out[k, :row_bytes] = r
    return out


def pack_samples(dataset, indices=None, workers: Optional[int] = None) -> PackedSamples:
    """Preprocess ``dataset[i]`` for ``i`` in ``indices`` (default: every sample) once, on at most
    ``workers`` host threads (default ``min(16, os.cpu_count())``), into the arrays of a device
    cache. Host only. ``dataset`` may be a ``torch.utils.data.Subset`` (what ``train_fraction``
    produces): it is unwrapped through ``.dataset`` / ``.indices``.

    A dataset with ``raw_item`` and no ``transform`` (``CellSegmentationDataset``) is stored as
    uint8 pixels + a per-sample (lo, den) table; any other dataset (``SyntheticDiscDataset``, one
    with a ``transform``, a user's own) as the float image ``__getitem__`` returns. A
    ``transform`` is therefore evaluated ONCE, at cache time, and must be deterministic: a random
    one would be frozen at its first draw (use the loader's ``augment`` instead). Masks are one
    bit per pixel when every value of every mask is exactly 0 or 1, float32 otherwise."""
    base, idx = _unwrap(dataset, indices)
    if not idx:
        raise ValueError("pack_samples: no samples")
    u8 = hasattr(base, "raw_item") and getattr(base, "transform", None) is None

    def one(i):
        if u8:
            img, mask = base.raw_item(i)
            img = np.ascontiguousarray(img, dtype=np.uint8)
            lo, hi = int(img.min()), int(img.max())
            norm = (np.float32(lo), np.float32(hi - lo) if hi > lo else np.float32(1e-8))
        else:
            img, mask = base[i]
            img = np.ascontiguousarray(torch.as_tensor(img).detach().cpu().numpy(), dtype=np.float32)
            norm = None
        mask = np.ascontiguousarray(torch.as_tensor(mask).detach().cpu().numpy())
        hw = tuple(img.shape[-2:])
        if img.ndim < 2 or img.size != hw[0] * hw[1] or mask.size != img.size:
            raise ValueError(f"pack_samples: sample {i} is not one H x W channel (image {img.shape}, mask {mask.shape})")
        binary = bool(np.all((mask == 0) | (mask == 1)))
        flat = mask.reshape(-1)
        packed = np.packbits(flat.astype(np.uint8), bitorder="little") if binary else flat.astype(np.float32).view(np.uint8)
        return img.reshape(-1).view(np.uint8), norm, packed, binary, hw

    n_workers = max(1, min(workers if workers is not None else default_workers(), len(idx)))
    if n_workers == 1:
        got = [one(i) for i in idx]
    else:
        with ThreadPoolExecutor(max_workers=n_workers) as pool:
            got = list(pool.map(one, idx))
    H, W = got[0][4]
    if any(g[4] != (H, W) for g in got):
        raise ValueError("pack_samples: samples differ in size")
    n = H * W
    bits = all(g[3] for g in got)
    if bits:
        mask_rows, mask_bytes = [g[2] for g in got], -(-n // 8)
    else:  # a binary sample's bits unpack to its exact 0.0 / 1.0 values
        mask_rows = [np.unpackbits(g[2], bitorder="little")[:n].astype(np.float32).view(np.uint8) if g[3] else g[2]
                     for g in got]
        mask_bytes = 4 * n
    return PackedSamples(image=_rows([g[0] for g in got], n if u8 else 4 * n), mask=_rows(mask_rows, mask_bytes),
                         norm=np.array([g[1] for g in got], np.float32).reshape(-1, 2) if u8 else None,
                         image_format="u8" if u8 else "f32", mask_format="bits" if bits else "f32", size=(H, W))


_AUGMENT_CODES = {None: 1, "flip": 4, "d4": 8}


def _resolve_augment(augment):
    """None, "flip", "d4" as they are; "affine" -> ``AffineAugment()``; an ``AffineAugment`` as it is."""
    if isinstance(augment, AffineAugment):
        return augment
    if isinstance(augment, str) and augment == "affine":
        return AffineAugment()
    if augment is None or (isinstance(augment, str) and augment in _AUGMENT_CODES):
        return augment
    raise ValueError(f"augment must be None, 'flip', 'd4', 'affine' or an AffineAugment, got {augment!r}")


def apply_symmetry(t: torch.Tensor, s: int) -> torch.Tensor:
    """Symmetry code ``s`` of ``pis_cache_batch`` on the last two dimensions: bit 0 flips W, bit 1
    flips H, then bit 2 transposes."""
    if s & 1:
        t = t.flip(-1)
    if s & 2:
        t = t.flip(-2)
    if s & 4:
        t = t.transpose(-1, -2)
    return t


class DeviceCachedLoader:
    """Batches of ANY map-style dataset assembled on the GPU from a device-resident cache.

    Construction preprocesses the whole dataset once with its unchanged host code
    (``pack_samples``: uint8 pixels + one bit per mask pixel for ``CellSegmentationDataset``, 36 KB
    per 128^2 sample) and uploads it in pinned chunks; the cache arrays are plain torch tensors on
    ``device``. EVERY RANK HOLDS THE FULL SET: the shards change with the epoch, so a rank needs any
    sample sooner or later. If the packed set exceeds ``max_bytes`` (default: a quarter of the
    device's free memory) a ``ValueError`` is raised before anything is allocated on the device.

    The order is ``DeviceDiscLoader``'s and ``DistributedSampler(seed=seed)``'s (``shard_indices``;
    ``set_epoch``, ``indices()``, ``len()``). At ``__iter__`` the epoch's index list and symmetry
    codes go to the device in one copy; each batch is a slice of them and one ``pis_cache_batch``
    launch on the current stream: no host work and no host-to-device copy per step. Batches are
    ``(images, masks)`` of shape (b, 1, H, W) float32 on ``device``, bit-identical to
    ``torch.stack`` of the dataset items, so ``train_epoch``, ``validate``, ``evaluate_model`` and
    ``StepGraph.step`` take them as they are.

    ``augment``: None (default), "flip" (codes 0-3: W and H flips) or "d4" (codes 0-7, adds the
    transpose; square sizes only). Sample ``i``'s code in an epoch is entry ``i`` of one
    ``torch.randint`` over the whole dataset from a generator seeded by (seed, epoch), so it does
    not depend on ``world``, ``rank`` or ``batch_size`` (``symmetry_codes``). "affine" or an
    ``AffineAugment``: a random rotation, scale, shift, flip, gain and bias per sample and epoch
    (``affine_params``, drawn the same way), resampled by ``pis_cache_batch_affine`` — bilinear image,
    nearest mask, reflected borders, in fixed point, so a batch equals ``PackedSamples.warp`` of its
    records bit for bit; ``augment`` then holds the ``AffineAugment``. A dataset ``transform`` is
    evaluated once, at cache time: it must be deterministic."""

    CHUNK_BYTES = 64 << 20

    def __init__(self, dataset, batch_size: int, shuffle: bool = True, seed: int = 42, rank: int = 0, world: int = 1,
                 drop_last: bool = False, device=None, workers: Optional[int] = None, max_bytes: Optional[int] = None,
                 augment: Union[None, str, AffineAugment] = None):
        from . import _hip  # noqa: F401  (fail early when the library is missing)
        augment = _resolve_augment(augment)
        self.dataset, self.batch_size, self.seed = dataset, batch_size, seed
        self.shuffle, self.rank, self.world, self.drop_last = shuffle, rank, world, drop_last
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.augment = augment
        self.epoch = 0
        self.ids = list(range(len(dataset)))
        packed = pack_samples(dataset, workers=workers)
        self.size, self.image_format, self.mask_format = packed.size, packed.image_format, packed.mask_format
        if augment == "d4" and self.size[0] != self.size[1]:
            raise ValueError(f"augment='d4' transposes: it needs square samples, got {self.size[0]} x {self.size[1]}")
        if self.affine and max(self.size) > AFFINE_MAX_SIZE:
            raise ValueError(f"augment='affine' takes samples up to {AFFINE_MAX_SIZE} pixels a side, got "
                             f"{self.size[0]} x {self.size[1]}")
        self.nbytes = packed.nbytes
        limit = self.default_max_bytes(self.device) if max_bytes is None else int(max_bytes)
        self.check_fits(self.nbytes, limit)
        self.image = self._upload(packed.image)
        self.mask = self._upload(packed.mask)
        self.norm = self._upload(packed.norm) if packed.norm is not None else None

    @staticmethod
    def default_max_bytes(device) -> Optional[int]:
        """A quarter of the device's free memory (None = no limit for a host 'device')."""
        device = torch.device(device)
        if device.type != "cuda":
            return None
        return torch.cuda.mem_get_info(device)[0] // 4

    @staticmethod
    def check_fits(nbytes: int, max_bytes: Optional[int]) -> None:
        if max_bytes is not None and nbytes > max_bytes:
            raise ValueError(f"DeviceCachedLoader: the packed dataset takes {nbytes} bytes, more than "
                             f"max_bytes = {max_bytes}")

    def _upload(self, arr: np.ndarray) -> torch.Tensor:
        src = torch.from_numpy(arr)
        if self.device.type != "cuda":
            return src.clone()
        dst = torch.empty(src.shape, dtype=src.dtype, device=self.device)
        if src.numel() == 0:
            return dst
        row = src[0].numel() * src.element_size()
        step = max(1, self.CHUNK_BYTES // row)
        pinned = torch.empty((min(step, src.shape[0]),) + tuple(src.shape[1:]), dtype=src.dtype, pin_memory=True)
        for k in range(0, src.shape[0], step):
            part = src[k:k + step]
            pinned[:part.shape[0]].copy_(part)
            dst[k:k + step].copy_(pinned[:part.shape[0]], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()  # the staging buffer is reused
        return dst

    @property
    def affine(self) -> bool:
        return isinstance(self.augment, AffineAugment)

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def indices(self):
        return shard_indices(self.ids, self.shuffle, self.seed, self.epoch, self.rank, self.world)

    def __len__(self):
        return _num_batches(len(self.indices()), self.batch_size, self.drop_last)

    def affine_params(self, epoch: Optional[int] = None) -> np.ndarray:
        """The ``AFFINE_RECORD`` of every dataset sample (dataset-index order) in ``epoch`` (default:
        the current one); ``.view(np.int32).reshape(-1, 8)`` is the kernel's view. Sample ``i``'s
        seven draws are row ``i`` of one ``torch.rand(N, 7, dtype=float64)`` from a generator seeded
        by (seed, epoch), so they do not depend on ``world``, ``rank`` or ``batch_size``. Without an
        affine ``augment``: identity records."""
        n = len(self.ids)
        if not self.affine:
            return affine_record(self.size, rotate=np.zeros(n))
        au = self.augment
        e = self.epoch if epoch is None else epoch
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + e)
        u = 2.0 * torch.rand(n, 7, generator=g, dtype=torch.float64).numpy() - 1.0  # uniform in [-1, 1)
        H, W = self.size
        return affine_record(self.size, rotate=u[:, 0] * au.rotate, scale=np.exp(u[:, 1] * np.log(au.scale)),
                             shift=np.stack([u[:, 2] * au.translate * W, u[:, 3] * au.translate * H], 1),
                             flip=(u[:, 4] < 0.0) & bool(au.flip), gain=1.0 + u[:, 5] * au.gain,
                             bias=u[:, 6] * au.bias)

    def symmetry_codes(self, epoch: Optional[int] = None) -> torch.Tensor:
        """uint8 code of every dataset sample (dataset-index order) in ``epoch`` (default: the
        current one); all zero without ``augment`` and under the affine one."""
        n = len(self.ids)
        k = 1 if self.affine else _AUGMENT_CODES[self.augment]
        if k == 1:
            return torch.zeros(n, dtype=torch.uint8)
        e = self.epoch if epoch is None else epoch
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + e)
        return torch.randint(0, k, (n,), generator=g, dtype=torch.uint8)

    def __iter__(self):
        from . import _hip
        _hip.require_cuda(self.image, "DeviceCachedLoader")
        idx = self.indices()
        m = len(idx)
        stop = m - (m % self.batch_size if self.drop_last else 0)
        if self.affine:
            # one host-to-device copy per epoch: a 32-byte record per entry (first: 16-byte aligned
            # at every batch), then the int64 index list
            plan = torch.empty(40 * m, dtype=torch.uint8, pin_memory=True)
            ids = torch.tensor(idx, dtype=torch.int64)
            rec = np.ascontiguousarray(self.affine_params()[ids.numpy()])
            plan[:32 * m].copy_(torch.from_numpy(rec.view(np.uint8).reshape(-1)))
            plan[32 * m:].view(torch.int64).copy_(ids)
            return self._batches(plan.to(self.device, non_blocking=True), m, stop)
        # one host-to-device copy per epoch: the int64 index list, then one symmetry byte per entry
        plan = torch.empty(8 * m + (m if self.augment else 0), dtype=torch.uint8, pin_memory=True)
        ids = torch.tensor(idx, dtype=torch.int64)
        plan[:8 * m].view(torch.int64).copy_(ids)
        if self.augment:
            plan[8 * m:].copy_(self.symmetry_codes()[ids])
        plan_d = plan.to(self.device, non_blocking=True)
        return self._batches(plan_d, m, stop)

    def _batches(self, plan_d: torch.Tensor, m: int, stop: int):
        from . import _hip
        H, W = self.size
        img_fmt = _hip.PIS_CACHE_IMG_U8 if self.image_format == "u8" else _hip.PIS_CACHE_IMG_F32
        mask_fmt = _hip.PIS_CACHE_MASK_BITS if self.mask_format == "bits" else _hip.PIS_CACHE_MASK_F32
        n, bs = self.image.shape[0], self.batch_size
        affine = self.affine
        if affine:
            rec_p, idx_p = plan_d.data_ptr(), plan_d.data_ptr() + 32 * m
        else:
            idx_p, sym_p = plan_d.data_ptr(), (plan_d.data_ptr() + 8 * m if self.augment else 0)
        for k in range(0, stop, bs):
            b = min(bs, m - k)
            img = torch.empty(b, 1, H, W, device=self.device)
            mask = torch.empty(b, 1, H, W, device=self.device)
            if affine:
                _hip.call("pis_cache_batch_affine", self.image.data_ptr(), img_fmt, self.image.stride(0),
                          self.mask.data_ptr(), mask_fmt, self.mask.stride(0), _hip.ptr(self.norm), idx_p + 8 * k,
                          rec_p + 32 * k, n, img.data_ptr(), mask.data_ptr(), b, H, W, _hip.stream_handle(self.device))
                yield img, mask
                continue
            _hip.call("pis_cache_batch", self.image.data_ptr(), img_fmt, self.image.stride(0), self.mask.data_ptr(),
                      mask_fmt, self.mask.stride(0), _hip.ptr(self.norm), idx_p + 8 * k, sym_p + k if sym_p else 0,
                      n, img.data_ptr(), mask.data_ptr(), b, H, W, _hip.stream_handle(self.device))
            yield img, mask
