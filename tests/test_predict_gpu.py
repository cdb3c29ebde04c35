"""Whole-image inference on the device (csrc/infer.hip through predict.py) against the numpy
definition of predict.py: the gather and the blend bit for bit (==), the blend against the float64
weighted mean within the bound of its rounding steps, the Predictor against the model run by hand on
the numpy tiles, clean_mask device == host, test-time augmentation in evaluate_model and the CLI.

The kernels give a thread a run of 4 output pixels: the 40 x 56 sources take the float4 path, 5 x 7,
1 x 1, 33 x 47 and 50 x 70 the scalar one; 16 x 16 tiles put several jobs' worth of threads in flight
per block row, 32 x 32 fills a 256-thread block exactly."""
import functools

import numpy as np
import pytest
import torch

from oracle import reference_torch as rt
from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd import evaluate as ev
from physics_informed_image_segmentation_amd import predict as pr

pytestmark = pytest.mark.gpu

H0, W0 = 40, 56
# (th, tw, ov, the sets of codes): the last tiling is not square, so the flip codes only
TILINGS = [(16, 16, 0, (0x01, 0x0F, 0xFF, 0xA4)), (16, 16, 8, (0x01, 0x0F, 0xFF, 0xA4)),
           (32, 32, 16, (0x01, 0x0F, 0xFF, 0xA4)), (16, 32, 8, (0x01, 0x0F, 0x04, 0x0A))]
THR = 0.5


@functools.lru_cache(maxsize=None)
def _sources(fmt, H=H0, W=W0, S=2):
    """(src numpy, norm numpy or None): seeded, S sources of H x W."""
    rng = np.random.default_rng(1234 + H * 100 + W)
    if fmt == "u8":
        src = rng.integers(3, 250, (S, H, W), dtype=np.uint8)
        lo = src.reshape(S, -1).min(1).astype(np.float32)
        hi = src.reshape(S, -1).max(1).astype(np.float32)
        return src, np.stack([lo, np.where(hi > lo, hi - lo, np.float32(1e-8))], 1).astype(np.float32)
    return rng.uniform(0.01, 0.99, (S, H, W)).astype(np.float32), None


def _gather_dev(src, plan, norm, **kw):
    out = pr.gather_tiles(torch.from_numpy(src).cuda(), plan, None if norm is None else torch.from_numpy(norm).cuda(), **kw)
    assert out.dtype == torch.float32 and out.is_contiguous()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _u(J, th, tw):
    return np.random.default_rng(J * 7 + th).uniform(0.01, 0.99, (J, 1, th, tw)).astype(np.float32)


def _cover_and_mean(u, plan, S):
    """(cover count c per pixel, float64 weighted mean), straight from the definition."""
    H, W, th, tw = plan.H, plan.W, plan.th, plan.tw
    wy, wx = pr.ramp_weights(th, plan.ov), pr.ramp_weights(tw, plan.ov)
    num, den, c = np.zeros((S, H, W)), np.zeros((S, H, W)), np.zeros((S, H, W), int)
    j = 0
    for s in range(S):
        for y0 in plan.oy:
            for x0 in plan.ox:
                hh, ww = min(th, H - y0), min(tw, W - x0)
                w = (wy[:hh, None] * wx[None, :ww]).astype(np.float64)
                for q in plan.codes:
                    v = pr.invert_symmetry_np(u[j, 0], q)[:hh, :ww].astype(np.float64)
                    num[s, y0:y0 + hh, x0:x0 + ww] += w * v
                    den[s, y0:y0 + hh, x0:x0 + ww] += w
                    c[s, y0:y0 + hh, x0:x0 + ww] += 1
                    j += 1
    return c, num / den


def _check_blend(u, plan, S):
    want_p, want_m = pr.blend_tiles_np(u, plan, S, THR)
    ud = torch.from_numpy(u).cuda()
    prob, mask = pr.blend_tiles(ud, plan, S, THR)
    assert prob.dtype == torch.float32 and mask.dtype == torch.uint8 and tuple(prob.shape) == (S, plan.H, plan.W)
    p, m = prob.cpu().numpy(), mask.cpu().numpy()
    np.testing.assert_array_equal(p, want_p)
    np.testing.assert_array_equal(m, (p > np.float32(THR)).astype(np.uint8))
    np.testing.assert_array_equal(m, want_m)
    again_p, again_m = pr.blend_tiles(ud, plan, S, THR)
    assert torch.equal(again_p, prob) and torch.equal(again_m, mask)
    only_p, none = pr.blend_tiles(ud, plan, S, THR, want_mask=False)      # mask == NULL
    assert none is None and torch.equal(only_p, prob)
    c, p64 = _cover_and_mean(u, plan, S)
    assert c.min() >= plan.Ns and c.max() <= 9 * plan.Ns
    err = np.abs(p.astype(np.float64) - p64)
    assert (err <= (c + 2) * 2.0 ** -24).all(), float((err / ((c + 2) * 2.0 ** -24)).max())
    return p


# ---------------------------------------------------------------------------- gather

@pytest.mark.parametrize("fmt", ["u8", "f32"])
@pytest.mark.parametrize("th, tw, ov, masks", TILINGS)
def test_gather_bit_for_bit(hip, th, tw, ov, masks, fmt):
    src, norm = _sources(fmt)
    for sym in masks:
        plan = pr.tile_plan(H0, W0, (th, tw), ov, sym)
        want = pr.gather_tiles_np(src, plan, norm)
        assert want.shape == (plan.jobs(2), 1, th, tw)
        np.testing.assert_array_equal(_gather_dev(src, plan, norm), want, err_msg=f"sym_mask {sym:#x}")


@pytest.mark.parametrize("fmt", ["u8", "f32"])
@pytest.mark.parametrize("H, W", [(5, 7), (1, 1)])
def test_gather_small_images_wrap(hip, H, W, fmt):
    src, norm = _sources(fmt, H, W, 2)
    plan = pr.tile_plan(H, W, (16, 16), 8, 0xFF)
    assert plan.jobs(2) == 16
    np.testing.assert_array_equal(_gather_dev(src, plan, norm), pr.gather_tiles_np(src, plan, norm))


def test_gather_in_chunks_that_split_a_symmetry_group(hip):
    src, norm = _sources("u8")
    plan = pr.tile_plan(H0, W0, (32, 32), 16, 0xFF)
    J = plan.jobs(2)
    want = pr.gather_tiles_np(src, plan, norm)
    cut = 8 * 3 + 5               # inside the fourth tile's group of 8
    a = _gather_dev(src, plan, norm, first_job=0, n_jobs=cut)
    b = _gather_dev(src, plan, norm, first_job=cut, n_jobs=J - cut)
    np.testing.assert_array_equal(np.concatenate([a, b]), want)
    one = _gather_dev(src, plan, norm, first_job=J - 1, n_jobs=1)
    np.testing.assert_array_equal(one, want[-1:])
    with pytest.raises(_hip.HipError):
        _gather_dev(src, plan, norm, first_job=J - 1, n_jobs=2)


# ---------------------------------------------------------------------------- blend

@pytest.mark.parametrize("th, tw, ov, masks", TILINGS)
def test_blend_bit_for_bit(hip, th, tw, ov, masks):
    for sym in masks:
        plan = pr.tile_plan(H0, W0, (th, tw), ov, sym)
        _check_blend(_u(plan.jobs(2), th, tw), plan, 2)


@pytest.mark.parametrize("H, W", [(5, 7), (1, 1), (33, 47)])
def test_blend_odd_sizes(hip, H, W):
    """W % 4 != 0: the scalar stores, and runs cut at the row's end."""
    plan = pr.tile_plan(H, W, (16, 16), 8, 0xFF)
    _check_blend(_u(plan.jobs(2), 16, 16), plan, 2)


def test_round_trip_returns_the_image(hip):
    """blend(gather(img)) under all eight symmetries: a gather and a blend that disagreed about a
    symmetry's inverse would mix pixels of different places."""
    src, _ = _sources("f32")
    for th, tw, ov in ((32, 32, 16), (16, 16, 8), (16, 16, 0)):
        plan = pr.tile_plan(H0, W0, (th, tw), ov, 0xFF)
        tiles = pr.gather_tiles(torch.from_numpy(src).cuda(), plan)
        prob, _ = pr.blend_tiles(tiles, plan, 2, THR)
        c, _ = _cover_and_mean(np.zeros((plan.jobs(2), 1, th, tw), np.float32), plan, 2)
        err = np.abs(prob.cpu().numpy().astype(np.float64) - src.astype(np.float64))
        assert (err <= (c + 2) * 2.0 ** -24).all(), float(err.max())


# ---------------------------------------------------------------------------- Predictor

@functools.lru_cache(maxsize=None)
def _net():
    from physics_informed_image_segmentation_amd import UNet
    torch.manual_seed(42)
    return UNet(1, 1, 64, dropout=0.0).cuda().eval()


def test_predictor_single_tile_is_the_model(hip):
    net = _net()
    x = rt.synthetic_batch(2, 64, 64, seed=3)[0].cuda()
    with torch.no_grad():
        want = net(x)
    for tile in (64, 512):
        prob, mask = pr.Predictor(net, tile=tile, overlap=16, tta=None).predict_batch(x)
        assert prob.shape == want.shape and prob.dtype == torch.float32 and mask.dtype == torch.uint8
        assert torch.equal(prob, want)
        assert torch.equal(mask, (want > 0.5).to(torch.uint8))


def test_predictor_d4_is_the_definition(hip):
    """80 x 96 under 64 x 64 tiles, overlap 16, all eight symmetries, chunks of 5 (the last chunk is
    pulled back and repeats three jobs): prob is blend_tiles_np of the tile outputs obtained by running
    the model on gather_tiles_np chunks of the same size and order."""
    net = _net()
    H, W = 80, 96
    img = rt.synthetic_batch(1, 96, 96, seed=5)[0][:, :, :H, :].contiguous()
    p = pr.Predictor(net, tile=64, overlap=16, tta="d4", batch_tiles=5)
    plan = p.plan(H, W)
    J = plan.jobs(1)
    assert (plan.th, plan.tw, J) == (64, 64, 32)
    n, starts = pr.chunk_starts(J, 5)
    u = np.empty((J, 1, 64, 64), np.float32)
    with torch.no_grad():
        for first in starts:
            tiles = pr.gather_tiles_np(img[:, 0].numpy(), plan, first_job=first, n_jobs=n)
            u[first:first + n] = net(torch.from_numpy(tiles).cuda()).cpu().numpy()
    want_p, want_m = pr.blend_tiles_np(u, plan, 1, 0.5)
    prob, mask = p.predict_batch(img.cuda())
    assert tuple(prob.shape) == (1, 1, H, W)
    np.testing.assert_array_equal(prob[:, 0].cpu().numpy(), want_p)
    np.testing.assert_array_equal(mask[:, 0].cpu().numpy(), want_m)


def test_predict_image_uint8_is_predict_batch_of_its_float_form(hip):
    net = _net()
    rng = np.random.default_rng(9)
    img = rng.integers(20, 230, (50, 70), dtype=np.uint8)
    p = pr.Predictor(net, tile=32, overlap=8, tta="flip", batch_tiles=7)
    prob, mask = p.predict_image(img)
    assert tuple(prob.shape) == (50, 70) and prob.is_cuda and mask.dtype == torch.uint8
    f = img.astype(np.float32)
    f = (f - f.min()) / (f.max() - f.min() + 1e-8)        # the dataset's whole-image min-max
    prob_b, mask_b = p.predict_batch(torch.from_numpy(f)[None, None].cuda())
    assert torch.equal(prob, prob_b[0, 0]) and torch.equal(mask, mask_b[0, 0])
    prob_f, _ = p.predict_image(img.astype(np.float64) * 3.0 + 1.0)      # a float image: normalised on the host
    assert prob_f.shape == prob.shape and bool(torch.isfinite(prob_f).all())
    small = pr.Predictor(net, tta="d4", max_workspace_bytes=1 << 16)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        small.predict_image(img)


# ---------------------------------------------------------------------------- clean_mask

def _discs_with_holes(B, H, W, seed):
    """Disc masks with a punched hole in every disc large enough, and single-pixel specks."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for _ in range(4):
            cy, cx, r = rng.uniform(6, H - 6), rng.uniform(6, W - 6), rng.uniform(4, 9)
            d2 = (y - cy) ** 2 + (x - cx) ** 2
            out[b][d2 <= r * r] = 1
            out[b][d2 <= (r / 3) ** 2] = 0
        for _ in range(6):
            out[b, rng.integers(0, H), rng.integers(0, W)] = 1
    return out


def _specks(B, H, W, seed):
    """Sparse noise (specks of a few pixels) around a thick frame-like ring with holes."""
    rng = np.random.default_rng(seed)
    out = (rng.random((B, H, W)) < 0.12).astype(np.uint8)
    out[:, 4:H - 4, 4:W - 4] |= (rng.random((B, H - 8, W - 8)) < 0.75).astype(np.uint8)
    return out


@pytest.mark.parametrize("name, make", [("discs 48x64", lambda: _discs_with_holes(2, 48, 64, 1)),
                                        ("specks 33x47", lambda: _specks(2, 33, 47, 2)),
                                        ("specks 64x64", lambda: _specks(2, 64, 64, 3))])
def test_clean_mask_device_is_host(hip, name, make):
    m = make()
    t = torch.from_numpy(m)
    for conn in (4, 8):
        host = pr.clean_mask(t, min_area=3, fill_holes=True, connectivity=conn).numpy()
        assert ((host == 1) & (m == 0)).any(), "no hole in the input"
        assert ((host == 0) & (m == 1)).any(), "no speck in the input"
        for min_area, fill in ((3, True), (0, True), (3, False), (10, True), (0, False)):
            want = pr.clean_mask(t, min_area=min_area, fill_holes=fill, connectivity=conn)
            got = pr.clean_mask(t.cuda(), min_area=min_area, fill_holes=fill, connectivity=conn)
            assert got.is_cuda and got.dtype == torch.uint8 and got.shape == t.shape
            assert torch.equal(got.cpu(), want), (name, conn, min_area, fill)
    # other input forms: a float (B, 1, H, W) mask and a single image
    want = pr.clean_mask(t, min_area=3, fill_holes=True)
    assert torch.equal(pr.clean_mask(t.float()[:, None].cuda(), 3, True).cpu()[:, 0], want)
    assert torch.equal(pr.clean_mask(t[0].cuda(), 3, True).cpu(), want[0])
    assert torch.equal(pr.clean_mask(t.cuda(), 3, True, backend="host").cpu(), want)


# ---------------------------------------------------------------------------- evaluate_model

def test_evaluate_model_tta(hip):
    net = _net()
    img, mask = rt.synthetic_batch(4, 64, 64, seed=7)
    loader = [(img[:2], mask[:2]), (img[2:], mask[2:])]
    dev = torch.device("cuda")
    base = ev.evaluate_model(net, loader, dev)
    off = ev.evaluate_model(net, loader, dev, tta=None)
    assert set(off) == set(base)
    for k in base:
        np.testing.assert_array_equal(off[k], base[k], err_msg=k)
    d4 = ev.evaluate_model(net, loader, dev, tta="d4", tta_tile=64, tta_overlap=16)
    assert set(d4) == set(base)
    for k in base:
        assert len(d4[k]) == len(base[k]) == 4
    assert np.isfinite(d4["dice_scores"]).all() and ((d4["dice_scores"] >= 0) & (d4["dice_scores"] <= 1)).all()
    with pytest.raises(ValueError):
        ev.evaluate_model(net, loader, dev, tta="rot")


# ---------------------------------------------------------------------------- CLI

def test_predict_cli(hip, tmp_path):
    from PIL import Image

    import predict as cli
    from physics_informed_image_segmentation_amd import UNet
    from physics_informed_image_segmentation_amd.evaluate_comparison import load_model
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.default_rng(11)
    sizes = {"a": (50, 70), "b": (64, 64), "c": (100, 40)}
    for stem, (H, W) in sizes.items():
        a = rng.integers(30, 90, (H, W), dtype=np.uint8)
        a[H // 4:H // 2, W // 4:W // 2] += 120
        Image.fromarray(a).save(src / f"{stem}.png")
    torch.manual_seed(1)
    ckpt = tmp_path / "m.pth"
    torch.save(UNet(1, 1, 64).state_dict(), ckpt)
    out = tmp_path / "out"
    written = cli.main(["--model", str(ckpt), "--input", str(src), "--output", str(out), "--tile", "64", "--overlap",
                        "16", "--tta", "flip", "--save-prob"])
    assert [p.name for p in written] == ["a_mask.png", "b_mask.png", "c_mask.png"]
    predictor = pr.Predictor(load_model(ckpt, torch.device("cuda")), tile=64, overlap=16, tta="flip")
    for stem, (H, W) in sizes.items():
        m = np.asarray(Image.open(out / f"{stem}_mask.png"))
        assert m.shape == (H, W) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255}
        prob = np.load(out / f"{stem}_prob.npy")
        assert prob.shape == (H, W) and prob.dtype == np.float32
        want_p, want_m = predictor.predict_image(np.asarray(Image.open(src / f"{stem}.png").convert("L")))
        np.testing.assert_array_equal(prob, want_p.cpu().numpy())
        np.testing.assert_array_equal(m, want_m.cpu().numpy() * 255)
    # clean-up and --resize: the mask keeps the input's size
    out2 = tmp_path / "out2"
    cli.main(["--model", str(ckpt), "--input", str(src / "a.png"), "--output", str(out2), "--resize", "64", "64",
              "--min-object-area", "4", "--fill-holes", "--connectivity", "4"])
    m = np.asarray(Image.open(out2 / "a_mask.png"))
    assert m.shape == (50, 70) and set(np.unique(m)) <= {0, 255}
    assert not (out2 / "a_prob.npy").exists()
