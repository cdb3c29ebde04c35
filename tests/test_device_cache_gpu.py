"""The device-resident dataset cache on the GPU: pis_cache_batch (csrc/cache.hip) against the
host dataset items, bit for bit, in every image format x mask format x symmetry; the loader's
order, sharding, augmentation and copy-free steps; epochs and evaluation fed by it equal to the
DataLoader path. The dataset is the COCO file of device_cache_fixture.py."""
import importlib

import pytest
import torch
from device_cache_fixture import make, symmetry
from torch.utils.data import DataLoader

from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd.dataset import DeviceCachedLoader, SyntheticDiscDataset, pack_samples

pytestmark = pytest.mark.gpu
tr = importlib.import_module("physics_informed_image_segmentation_amd.train")

KINDS = ["u8-bits", "u8-f32", "f32-bits", "f32-f32"]
# (N, B, H, W) and the batch's sample indices
SHAPES = [((7, 5, 5, 7), [6, 2, 0, 4, 3]),     # 35 pixels: mask word tail, W % 4 != 0, padded strides
          ((7, 1, 16, 16), [4]),                # square: the transpose codes
          ((7, 5, 16, 48), [1, 2, 5, 6, 4]),    # non-square: flips only
          ((3, 4, 32, 80), [2, 0, 2, 1])]       # a repeated index inside the batch
FMT = {"u8": _hip.PIS_CACHE_IMG_U8, "f32": _hip.PIS_CACHE_IMG_F32}
MFMT = {"bits": _hip.PIS_CACHE_MASK_BITS, "f32": _hip.PIS_CACHE_MASK_F32}


class _Cache:
    """A packed dataset on the device and its host items (computed once per dataset)."""

    def __init__(self, ds):
        self.items = [ds[i] for i in range(len(ds))]
        pk = pack_samples(ds, workers=2)
        self.pk, self.size = pk, pk.size
        self.image, self.mask = torch.from_numpy(pk.image).cuda(), torch.from_numpy(pk.mask).cuda()
        self.norm = torch.from_numpy(pk.norm).cuda() if pk.norm is not None else None

    def run(self, idx, sym=None, n=None, rc=False):
        H, W = self.size
        B = len(idx)
        idx_d = torch.tensor(idx, dtype=torch.int64).cuda()
        sym_d = torch.tensor(sym, dtype=torch.uint8).cuda() if sym is not None else None
        img = torch.full((B, 1, H, W), 7.0, device="cuda")
        mask = torch.full((B, 1, H, W), 7.0, device="cuda")
        args = (self.image.data_ptr(), FMT[self.pk.image_format], self.image.stride(0), self.mask.data_ptr(),
                MFMT[self.pk.mask_format], self.mask.stride(0), _hip.ptr(self.norm), idx_d.data_ptr(), _hip.ptr(sym_d),
                len(self.items) if n is None else n, img.data_ptr(), mask.data_ptr(), B, H, W, _hip.stream_handle())
        if rc:
            return _hip.lib().pis_cache_batch(*args)
        _hip.call("pis_cache_batch", *args)
        torch.cuda.synchronize()
        return img.cpu(), mask.cpu()

    def want(self, idx, sym=None):
        sym = [0] * len(idx) if sym is None else sym
        return (torch.stack([symmetry(self.items[i][0], s) for i, s in zip(idx, sym)]),
                torch.stack([symmetry(self.items[i][1], s) for i, s in zip(idx, sym)]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,idx", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_kernel_bitwise_equal_to_host_items(hip, tmp_path, kind, shape, idx):
    N, B, H, W = shape
    c = _Cache(make(kind, tmp_path, (W, H), n=N))
    assert c.size == (H, W) and len(c.items) == N and len(idx) == B
    assert (c.pk.image_format, c.pk.mask_format) == tuple(kind.split("-"))
    codes = range(8) if H == W else range(4)
    cases = [None] + [[s] * B for s in codes] + [[list(codes)[(3 * j + 1) % len(codes)] for j in range(B)]]
    for sym in cases:
        img, mask = c.run(idx, sym)
        w_img, w_mask = c.want(idx, sym)
        assert img.shape == (B, 1, H, W) and torch.equal(img, w_img), (kind, sym)
        assert torch.equal(mask, w_mask), (kind, sym)
    if N > 2 and 2 in idx and kind.startswith("u8"):
        img, _ = c.run(idx)
        assert torch.count_nonzero(img[idx.index(2)]) == 0  # the constant image: (v - lo) / 1e-8 = 0


def test_kernel_illegal_entries_are_nan_not_read(hip, tmp_path):
    c = _Cache(make("u8-bits", tmp_path, (48, 16)))
    idx = [3, -1, 7, 1 << 40, 5]
    img, mask = c.run(idx)
    w_img, w_mask = c.want([3, 5])
    assert torch.equal(img[[0, 4]], w_img) and torch.equal(mask[[0, 4]], w_mask)
    assert img[1:4].isnan().all() and mask[1:4].isnan().all()
    # transpose on a non-square grid and a code above 7: NaN for that entry only
    img, mask = c.run([0, 1, 2], [4, 1, 9])
    assert img[[0, 2]].isnan().all() and mask[[0, 2]].isnan().all()
    assert torch.equal(img[1], c.want([1], [1])[0][0]) and torch.equal(mask[1], c.want([1], [1])[1][0])
    c5 = _Cache(make("f32-f32", tmp_path / "odd", (7, 5)))  # the per-pixel kernel
    img, mask = c5.run([7, 6])
    assert img[0].isnan().all() and mask[0].isnan().all() and torch.equal(img[1], c5.items[6][0])
    # a smaller N than the cache: rows beyond it are out of range
    img, _ = c.run([2, 3], n=3)
    assert not img[0].isnan().any() and img[1].isnan().all()


def test_kernel_argument_errors(hip, tmp_path):
    c = _Cache(make("u8-bits", tmp_path, (48, 16)))
    good = c.run([0], rc=True)
    assert good == 0
    lib = _hip.lib()
    H, W = c.size
    idx_d = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.empty(2, 1, H, W, device="cuda")

    def rc(img_fmt=0, img_stride=None, mask_fmt=0, mask_stride=None, norm=c.norm.data_ptr(), shift=0):
        return lib.pis_cache_batch(c.image.data_ptr() + shift, img_fmt, img_stride or c.image.stride(0),
                                   c.mask.data_ptr(), mask_fmt, mask_stride or c.mask.stride(0), norm, idx_d.data_ptr(),
                                   0, 7, out[0].data_ptr(), out[1].data_ptr(), 1, H, W, _hip.stream_handle())
    assert rc() == 0
    assert rc(img_fmt=2) == -1 and b"image format" in lib.pis_last_error()
    assert rc(mask_fmt=5) == -1
    assert rc(img_stride=H * W + 8) == -1 and b"stride" in lib.pis_last_error()
    assert rc(img_stride=H * W - 16) == -1
    assert rc(mask_stride=H * W // 8 - 16) == -1
    assert rc(norm=0) == -1
    assert rc(shift=4) == -1 and b"aligned" in lib.pis_last_error()
    assert rc(img_fmt=1) == -1  # f32 rows do not fit the u8 stride
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cell(tmp_path_factory):
    ds = make("u8-bits", tmp_path_factory.mktemp("cell"), (48, 16))
    return ds, [ds[i] for i in range(len(ds))]


def _stack(items, idx, codes=None, which=0):
    return torch.stack([symmetry(items[i][which], 0 if codes is None else int(codes[i])) for i in idx])


@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_batches_equal_host_items(hip, cell, drop_last):
    ds, items = cell
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        ld = DeviceCachedLoader(ds, 3, shuffle=True, seed=5, rank=rank, world=world, drop_last=drop_last)
        assert ld.dataset is ds and (ld.image_format, ld.mask_format) == ("u8", "bits")
        seen = []
        for epoch in (0, 1):
            ld.set_epoch(epoch)
            idx = ld.indices()
            seen.append(idx)
            batches = list(ld)
            assert len(batches) == len(ld) == (len(idx) // 3 if drop_last else -(-len(idx) // 3))
            for k, (img, mask) in enumerate(batches):
                part = idx[3 * k:3 * k + 3]
                assert img.device.type == "cuda" and img.is_contiguous() and img.dtype == torch.float32
                assert torch.equal(img.cpu(), _stack(items, part)) and torch.equal(mask.cpu(), _stack(items, part, which=1))
                assert img.to(img.device) is img  # already resident: the step's .to(device) is a no-op
        assert seen[0] != seen[1]


def test_loader_flip_augmentation(hip, cell):
    ds, items = cell
    ld = DeviceCachedLoader(ds, 4, shuffle=True, seed=3, augment="flip")
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        codes, idx = ld.symmetry_codes(epoch), ld.indices()
        got = list(ld)
        img, mask = torch.cat([b[0] for b in got]).cpu(), torch.cat([b[1] for b in got]).cpu()
        assert torch.equal(img, _stack(items, idx, codes)) and torch.equal(mask, _stack(items, idx, codes, which=1))
    assert codes.any()


def test_loader_d4_augmentation_square(hip, tmp_path):
    ds = make("f32-bits", tmp_path, (16, 16))
    items = [ds[i] for i in range(len(ds))]
    ld = DeviceCachedLoader(ds, 7, shuffle=False, seed=1, augment="d4")
    codes = ld.symmetry_codes()
    img, mask = next(iter(ld))
    assert int(codes.max()) >= 4
    assert torch.equal(img.cpu(), _stack(items, range(7), codes)) and torch.equal(mask.cpu(), _stack(items, range(7), codes, 1))


def test_loader_steps_enqueue_no_host_to_device_copy(hip, cell, monkeypatch):
    ds, _ = cell
    ld = DeviceCachedLoader(ds, 2, shuffle=True, seed=5, augment="flip")
    calls, copies = [], []

    class Tracer:
        def begin(self, name, args):
            calls.append(name)

        def end(self, tok):
            pass

    to, copy_ = torch.Tensor.to, torch.Tensor.copy_
    it = iter(ld)  # the epoch's one copy (index list + symmetry codes) happens here
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: (copies.append("to"), to(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *a, **k: (copies.append("copy_"), copy_(self, *a, **k))[1])
    _hip.set_tracer(Tracer())
    try:
        n = sum(1 for _ in it)
    finally:
        _hip.set_tracer(None)
        monkeypatch.undo()
    assert n == 4 and calls == ["pis_cache_batch"] * 4 and copies == []


def _epoch_pair(loader, seed=42):
    from physics_informed_image_segmentation_amd import AdamW, DiceBCEPDELoss, UNet
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    net = UNet(1, 1, 64).cuda()
    crit = DiceBCEPDELoss(pde_weight=1e-2, phase_field_weight=1e-2, diffusion_coeff=5.0, reaction_threshold=0.5,
                          epsilon=0.05).cuda()
    opt = AdamW(net.parameters(), lr=1e-4, weight_decay=1e-5)
    dev = torch.device("cuda", torch.cuda.current_device())
    va = tr.validate(net, loader, crit, dev, return_components=True)
    te = tr.train_epoch(net, loader, crit, opt, dev, return_components=True)
    torch.cuda.synchronize()
    return va, te, net.arena.detach().cpu().clone()


def test_epochs_equal_the_dataloader_path(hip, tmp_path):
    ds = make("u8-bits", tmp_path, (32, 32), n=6)
    va0, te0, w0 = _epoch_pair(DataLoader(ds, batch_size=2, shuffle=False))
    ld = DeviceCachedLoader(ds, 2, shuffle=False)
    assert len(ld) == 3
    va1, te1, w1 = _epoch_pair(ld)
    print("validate", va0, va1, "\ntrain_epoch", te0, te1, "\narena max |diff|", (w0 - w1).abs().max().item())
    assert va0 == va1 and te0 == te1
    assert torch.equal(w0, w1)


def test_evaluate_on_test_set_device_cache(hip, tmp_path):
    import numpy as np

    from device_cache_fixture import write_coco
    from physics_informed_image_segmentation_amd import UNet, evaluate_on_test_set
    img_dir, ann = write_coco(tmp_path)
    torch.manual_seed(1)
    net = UNet(1, 1, 64).cuda()
    dev = torch.device("cuda")
    a = evaluate_on_test_set(net, img_dir, ann, dev, batch_size=3)
    b = evaluate_on_test_set(net, img_dir, ann, dev, batch_size=3, device_cache=True)
    assert set(a) == set(b) and len(a["dice_scores"]) == 7
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_train_entry_point_with_device_cache(hip, tmp_path, capsys):
    model, result = tr.train(synthetic=(8, 4, 32, 32), device_data=False, device_cache=True, stage1_epochs=1,
                             stage2_epochs=1, base_dir=str(tmp_path))
    assert len(result["stage2"][2]) == 1 and 0.0 <= result["stage2"][2][0]["val_dice_score"] <= 1.0
    assert "falling back" not in capsys.readouterr().out


def test_ablation_variant_with_device_cache(hip, tmp_path, monkeypatch):
    from physics_informed_image_segmentation_amd import ablation as ab
    made = []
    init = DeviceCachedLoader.__init__
    monkeypatch.setattr(DeviceCachedLoader, "__init__",
                        lambda self, *a, **k: (made.append((k["shuffle"], k["augment"])), init(self, *a, **k))[1])
    res = ab.run_ablation_study("R1", [ab.define_ablation_r1()[3]], ab.DataSpec(synthetic=(4, 2, 2, 32, 32)),
                                device=torch.device("cuda"), batch_size=2, stage1_epochs=1, stage2_epochs=1,
                                output_dir=tmp_path, num_workers=0, device_cache=True, augment="flip")
    assert len(res["results"][0]["in_dist_metrics"]["dice_scores"]) == 2
    assert made == [(True, "flip"), (False, None), (False, None), (False, None)]  # augment: the training loader only
    with pytest.raises(ValueError, match="device_cache"):
        ab.run_ablation_variant(ab.define_ablation_r1()[3], ab.DataSpec(synthetic=(4, 2, 2, 32, 32)), augment="flip")


def test_train_falls_back_when_the_cache_does_not_fit(hip, monkeypatch):
    monkeypatch.setattr(DeviceCachedLoader, "default_max_bytes", staticmethod(lambda device: 100))
    said = []
    ds = SyntheticDiscDataset(4, (8, 8), seed=1)
    assert tr._cached_loaders(ds, ds, 2, 1, 0, torch.device("cuda"), 42, None, said.append) is None
    assert "falling back" in said[0] and "100" in said[0]
