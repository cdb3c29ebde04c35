"""Host side of the affine augmentation of the device cache: the records a loader draws
(DeviceCachedLoader.affine_params), the definition of the resampling (PackedSamples.warp) against
plain array operations, pis_cache_batch_affine's argument checks, the loader's and the CLIs'
acceptance of the new mode. No GPU. The datasets are those of device_cache_fixture.py."""
import numpy as np
import pytest
import torch
from device_cache_fixture import make
from torch.utils.data import Dataset

from physics_informed_image_segmentation_amd.dataset import (AFFINE_RECORD, AffineAugment, DeviceCachedLoader,
                                                             SyntheticDiscDataset, affine_record, pack_samples,
                                                             reflect_index)

KINDS = ["u8-bits", "u8-f32", "f32-bits", "f32-f32"]
SIZES = [(7, 5), (16, 16), (48, 16)]  # PIL (W, H)
IDENTITY = [65536, 0, 0, 0, 65536, 0, 0x3F800000, 0]  # a[6], 1.0f, 0.0f


def test_affine_params():
    ds = SyntheticDiscDataset(40, (8, 12), seed=9)
    mk = lambda **kw: DeviceCachedLoader(ds, kw.pop("bs", 2), seed=kw.pop("seed", 7), device="cpu",
                                         augment=kw.pop("augment", "affine"), **kw)
    a = mk()
    p0, p1 = a.affine_params(0), a.affine_params(1)
    assert p0.dtype == AFFINE_RECORD and p0.shape == (40,) and AFFINE_RECORD.itemsize == 32
    v0 = p0.view(np.int32).reshape(-1, 8)  # the kernel's view
    assert v0.shape == (40, 8) and np.array_equal(v0[:, :6], p0["a"])
    assert np.array_equal(v0[:, 6:].view(np.float32), np.stack([p0["gain"], p0["bias"]], 1))
    assert np.array_equal(p0, mk().affine_params(0))                       # reproducible
    assert not np.array_equal(p0, p1)                                      # per epoch
    assert not np.array_equal(p0, mk(seed=8).affine_params(0))             # per seed
    for kw in (dict(world=2, rank=1), dict(world=3, rank=0), dict(bs=5), dict(shuffle=False, drop_last=True)):
        assert np.array_equal(mk(**kw).affine_params(1), p1), kw
    a.set_epoch(1)
    assert np.array_equal(a.affine_params(), p1)                           # default: the current epoch
    assert not a.symmetry_codes().any()
    # the draws stay inside the default ranges: |A^-1| = 1 / scale, gain 1 +- 0.1, bias +- 0.05
    det = (p0["a"][:, 0].astype(np.float64) * p0["a"][:, 4] - p0["a"][:, 1].astype(np.float64) * p0["a"][:, 3]) / 2.0 ** 32
    assert np.all(np.abs(det) <= 1.25 ** 2 * 1.001) and np.all(np.abs(det) >= 1.25 ** -2 / 1.001)
    assert (det < 0).any() and (det > 0).any()                             # flips are drawn
    assert np.all(np.abs(p0["gain"] - 1) <= np.float32(0.1)) and np.all(np.abs(p0["bias"]) <= np.float32(0.05))
    # all ranges zero: the identity record for every sample, bit for bit
    for epoch in (0, 3):
        z = mk(augment=AffineAugment(rotate=0.0, scale=1.0, translate=0.0, flip=False, gain=0.0, bias=0.0))
        assert np.array_equal(z.affine_params(epoch).view(np.int32).reshape(-1, 8), np.tile(IDENTITY, (40, 1)))
    assert np.array_equal(mk(augment=None).affine_params(0).view(np.int32).reshape(-1, 8), np.tile(IDENTITY, (40, 1)))
    with pytest.raises(ValueError, match="int32"):
        affine_record((8, 12), scale=1e-5)


def test_reflect_index():
    assert np.array_equal(reflect_index(np.arange(-9, 9), 1), np.zeros(18, np.int64))
    want = np.pad(np.arange(5), 20, mode="reflect")  # ... 2 1 | 0 1 2 3 4 | 3 2 ..., five periods a side
    assert np.array_equal(reflect_index(np.arange(-20, 25), 5), want)
    assert np.array_equal(reflect_index(np.arange(-6, 8), 2), np.arange(-6, 8) % 2)
    period = np.concatenate([np.arange(4096), np.arange(4094, 0, -1)])  # 0 .. 4095, 4094 .. 1
    far = np.array([-(1 << 29), -(1 << 29) + 5000, (1 << 29) + 3, (1 << 29) + 4100, -1, 4096, 8190])
    assert np.array_equal(reflect_index(far, 4096), period[far % 8190])


@pytest.mark.parametrize("kind", KINDS)
def test_warp_against_array_operations(tmp_path, kind):
    for W, H in SIZES:
        ds = make(kind, tmp_path / f"{W}x{H}", (W, H), n=5)
        pk = pack_samples(ds, workers=1)
        assert (pk.image_format, pk.mask_format) == tuple(kind.split("-"))
        rec = lambda **kw: affine_record((H, W), **kw)
        same = lambda got, img, mask: (np.array_equal(got[0][0].numpy(), img), np.array_equal(got[1][0].numpy(), mask))
        for i in range(len(pk)):
            img, mask = (t[0].numpy() for t in pk.unpack(i))
            assert torch.equal(pk.warp(i, rec())[0], pk.unpack(i)[0]) and torch.equal(pk.warp(i, rec())[1], pk.unpack(i)[1])
            assert torch.equal(pk.warp(i, np.array(IDENTITY, np.int32))[0], pk.unpack(i)[0])  # the (8,) int32 view
            assert same(pk.warp(i, rec(flip=True)), img[:, ::-1], mask[:, ::-1]) == (True, True), (W, H, i)
            assert same(pk.warp(i, rec(rotate=180.0)), img[::-1, ::-1], mask[::-1, ::-1]) == (True, True), (W, H, i)
            if H == W:
                assert same(pk.warp(i, rec(rotate=90.0)), np.rot90(img, 3), np.rot90(mask, 3)) == (True, True), i
                assert same(pk.warp(i, rec(rotate=-90.0)), np.rot90(img, 1), np.rot90(mask, 1)) == (True, True), i
            # the content moves 3 right and 2 up; what enters is the reflection
            crop = lambda t: np.pad(t, 3, mode="reflect")[3 + 2:3 + 2 + H, 3 - 3:3 - 3 + W]
            assert same(pk.warp(i, rec(shift=(3.0, -2.0))), crop(img), crop(mask)) == (True, True), (W, H, i)
            g, b = np.float32(1.07), np.float32(-0.03)
            assert same(pk.warp(i, rec(gain=g, bias=b)), g * img + b, mask) == (True, True), (W, H, i)
            # half a pixel: the mean of two neighbours (u8: of the grey values, before the min-max)
            got = pk.warp(i, rec(shift=(-0.5, 0.0)))[0][0].numpy()
            if pk.image_format == "f32":
                nxt = np.concatenate([img[:, 1:], img[:, -2:-1]], 1)
                assert np.array_equal(got, (np.float32(32768) * img + np.float32(32768) * nxt) * np.float32(2.0 ** -16))
            else:
                raw = pk.image[i, :H * W].reshape(H, W).astype(np.float32)
                nxt = np.concatenate([raw[:, 1:], raw[:, -2:-1]], 1)
                lo, den = pk.norm[i]
                assert np.array_equal(got, ((raw + nxt) * np.float32(0.5) - lo) / den)


class _Row(Dataset):
    """Three 1 x 8 samples (H = 1: every row index reflects to 0), f32 image outside [0, 1]."""

    def __len__(self):
        return 3

    def __getitem__(self, i):
        x = torch.arange(8, dtype=torch.float32)
        return (3.0 * x - 5.0 + i).reshape(1, 1, 8), (x % (i + 2) == 0).float().reshape(1, 1, 8)


def test_warp_single_row_and_unclamped_values():
    pk = pack_samples(_Row())
    assert pk.size == (1, 8) and (pk.image_format, pk.mask_format) == ("f32", "bits")
    for i in range(3):
        img, mask = pk.unpack(i)
        assert torch.equal(pk.warp(i, affine_record((1, 8)))[0], img) and float(img.min()) < 0.0 < 1.0 < float(img.max())
        for dy in (-7.0, 5.0, 1000.0):  # any row is row 0
            got = pk.warp(i, affine_record((1, 8), shift=(0.0, dy)))
            assert torch.equal(got[0], img) and torch.equal(got[1], mask)
        # source x = 28 - x_out, two periods out: the reflection about pixel 0 undoes the flip
        got = pk.warp(i, affine_record((1, 8), flip=True, shift=(21.0, 0.0)))
        assert torch.equal(got[0], img) and torch.equal(got[1], mask)


def test_kernel_argument_errors_need_no_gpu():
    """What the host can know is PIS_ERR_ARG before any launch (the pointers are never read)."""
    from physics_informed_image_segmentation_amd import _hip
    lib = _hip.lib()
    p = 1 << 20  # a 16-byte aligned non-null stand-in

    def rc(img_fmt=0, img_stride=48, mask_fmt=0, mask_stride=16, norm=p, n=3, B=2, H=5, W=7, img=p, params=p):
        return lib.pis_cache_batch_affine(img, img_fmt, img_stride, p, mask_fmt, mask_stride, norm, p, params, n, p, p,
                                          B, H, W, 0)
    assert rc(params=0) == -1 and b"pis_cache_batch_affine" in lib.pis_last_error() and b"params" in lib.pis_last_error()
    assert rc(params=p + 8) == -1 and b"aligned" in lib.pis_last_error()
    assert rc(img_fmt=2) == -1 and b"image format" in lib.pis_last_error()
    assert rc(mask_fmt=-1) == -1 and b"mask format" in lib.pis_last_error()
    assert rc(img_stride=40) == -1 and b"stride" in lib.pis_last_error()  # no multiple of 16
    assert rc(img_stride=32) == -1                                         # shorter than 35 pixels
    assert rc(img_fmt=1, img_stride=128) == -1                             # 35 floats need 140 bytes
    assert rc(mask_fmt=1, mask_stride=128) == -1
    assert rc(norm=0) == -1
    assert rc(img=p + 4) == -1 and b"aligned" in lib.pis_last_error()
    assert rc(n=0) == -1 and rc(B=0) == -1 and rc(B=70000) == -1 and rc(W=0) == -1
    big = dict(img_stride=4097 * 16, mask_stride=4097 * 16 // 8 + 16 - (4097 * 16 // 8) % 16)
    assert rc(H=4097, W=16, **big) == -1 and b"4096" in lib.pis_last_error()
    assert rc(H=16, W=4097, **big) == -1 and b"4096" in lib.pis_last_error()


def test_loader_accepts_affine():
    ds = SyntheticDiscDataset(3, (4, 6), seed=1)
    ld = DeviceCachedLoader(ds, 2, device="cpu", augment="affine")
    assert ld.augment == AffineAugment() and ld.affine and len(ld) == 2
    mine = AffineAugment(rotate=10.0, flip=False)
    ld = DeviceCachedLoader(ds, 2, device="cpu", augment=mine)
    assert ld.augment is mine and ld.affine
    assert not DeviceCachedLoader(ds, 2, device="cpu", augment="flip").affine
    assert not DeviceCachedLoader(ds, 2, device="cpu").affine
    for bad in ("rot", "Affine", 3, AffineAugment):
        with pytest.raises(ValueError, match="augment"):
            DeviceCachedLoader(SyntheticDiscDataset(3, (4, 4), seed=1), 2, device="cpu", augment=bad)
    with pytest.raises(ValueError):
        AffineAugment(scale=0.0)


def test_train_and_ablation_need_the_device_cache():
    import importlib

    from physics_informed_image_segmentation_amd import ablation as ab
    tr = importlib.import_module("physics_informed_image_segmentation_amd.train")
    with pytest.raises(ValueError, match="device_cache"):
        tr.train(augment="affine")
    with pytest.raises(ValueError, match="device_cache"):
        ab.run_ablation_variant(ab.define_ablation_r1()[3], ab.DataSpec(synthetic=(4, 2, 2, 32, 32)),
                                augment=AffineAugment())


def test_cli_flags_parse():
    import evaluate as eval_cli
    import main
    a = main.parse_args(["--device-cache", "--augment", "affine"])
    assert a.device_cache and a.augment == "affine"
    with pytest.raises(SystemExit):
        main.parse_args(["--augment", "affine"])
    assert eval_cli.parse_args(["--baseline", "b", "--pde", "p", "--augment", "affine"]).augment == "affine"
