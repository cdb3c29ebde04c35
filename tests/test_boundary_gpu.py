"""Boundary F1 / Hausdorff on the device (csrc/boundary.hip through evaluate.py) against the host
path of evaluate.py on .cpu() copies. Everything in these metrics is integer geometry, so
boundary maps, counters and Hausdorff values are compared with ==; only the float32 F1 scores
(the same expression on the same integers, float32 on the host, float64 on the device) get 1e-6.

The label kernel's tile is 32 x 32, so the labelling cases also run at 100 x 131 (three tiles
plus a remainder down, four plus a remainder across) beside 33 x 47 and 80 x 144."""
import functools
import importlib

import numpy as np
import pytest
import torch
from scipy import ndimage

from oracle import reference_torch as rt
from physics_informed_image_segmentation_amd import evaluate as ev

pytestmark = pytest.mark.gpu
TILE = 32
TOLERANCES = (0, 1, 2, 3, 5)


# ---------------------------------------------------------------------------- host oracle

def _host_maps(fg: np.ndarray) -> np.ndarray:
    return np.stack([ev.extract_boundaries(m.astype(np.float32)) for m in fg]).astype(np.uint8)


def _host_counts(bp: np.ndarray, bt: np.ndarray, tol: int) -> np.ndarray:
    """(B, 4): |Bp|, |Bt|, sum(near_t * pred_b), sum(near_p * target_b) as _boundary_f1_np forms them."""
    out = []
    for p, t in zip(bp.astype(np.float32), bt.astype(np.float32)):
        near_t, near_p = ev._near(t > 0, tol), ev._near(p > 0, tol)
        out.append([p.sum(), t.sum(), (near_t * p).sum(), (near_p * t).sum()])
    return np.array(out, np.int64)


def _device(p: torch.Tensor, t: torch.Tensor, thr: float, tol: int):
    counts, bp, bt = ev._boundary_device(p.cuda(), t.cuda(), thr, tol, maps=True)
    return counts.cpu().numpy(), bp.cpu().numpy(), bt.cpu().numpy()


def _check_exact(p: torch.Tensor, t: torch.Tensor, thr: float, tolerances=TOLERANCES):
    """Maps, the four counters at every tolerance and the Hausdorff distances of a (B, H, W) pair."""
    B = p.shape[0]
    hp = _host_maps((p > thr).numpy())
    ht = _host_maps((t > 0).numpy())
    for tol in tolerances:
        counts, bp, bt = _device(p, t, thr, tol)
        np.testing.assert_array_equal(bp, hp)
        np.testing.assert_array_equal(bt, ht)
        np.testing.assert_array_equal(counts[:, :4], _host_counts(hp, ht, tol), err_msg=f"tolerance {tol}")
    hd = ev.compute_hausdorff_distance_batch(p.cuda(), t.cuda(), thr)
    assert hd.dtype == torch.float64 and hd.is_cuda
    hd = hd.cpu().numpy()
    for i in range(B):
        want = ev.compute_hausdorff_distance(p[i:i + 1, None], t[i:i + 1, None], thr)
        assert hd[i] == want, (i, hd[i], want)
        assert ev.compute_hausdorff_distance(p[i:i + 1, None].cuda(), t[i:i + 1, None].cuda(), thr) == want
    return hd


# ---------------------------------------------------------------------------- 1. known contours

def _known_shapes():
    def canvas():
        return np.zeros((12, 12), np.float32)
    sq = canvas()
    sq[2:7, 2:7] = 1
    full = np.ones((12, 12), np.float32)
    one = canvas()
    one[2, 2] = 1
    hole = canvas()
    hole[1:10, 1:10] = 1
    hole[3:8, 3:8] = 0
    hole[5, 5] = 1
    stair = canvas()
    stair[1:5, 1:5] = 1
    stair[1, 1] = 0
    return np.stack([sq, full, one, canvas(), hole, stair])


def test_known_contours():
    m = _known_shapes()
    want = _host_maps(m > 0)
    # the contours the host tests pin: ring of the square, image border, the pixel itself, nothing,
    # the outer ring only (hole border and nested island dropped), staircase corner interior
    assert want[0].sum() == 16 and want[1].sum() == 44 and want[2].sum() == 1 and want[3].sum() == 0
    assert want[4].sum() == 32 and want[4][5, 5] == 0 and want[5][2, 2] == 0 and want[5][1, 2] == 1
    got = ev.extract_boundaries_device(torch.from_numpy(m).cuda())
    assert got.dtype == torch.uint8 and got.shape == (6, 12, 12)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # (B, 1, H, W) input, and as prediction / target of one call
    got4 = ev.extract_boundaries_device(torch.from_numpy(m)[:, None].cuda())
    np.testing.assert_array_equal(got4.cpu().numpy(), want)
    _, bp, bt = _device(torch.from_numpy(m) * 0.9, torch.from_numpy(m[::-1].copy()), 0.5, 2)
    np.testing.assert_array_equal(bp, want)
    np.testing.assert_array_equal(bt, want[::-1])


# ---------------------------------------------------------------------------- 2. labelling worst cases

def _spiral(H: int, W: int, sealed: bool) -> np.ndarray:
    """All foreground but a one-pixel background corridor spiralling from (1, 1) to the centre,
    opened to the frame through (0, 1) unless ``sealed`` (then all of it is a hole)."""
    fg = np.ones((H, W), bool)

    def inside(y, x):
        return 1 <= y <= H - 2 and 1 <= x <= W - 2
    if not inside(1, 1):
        return fg
    y, x, d = 1, 1, 0
    fg[1, 1] = False
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while True:
        for turn in (0, 1):
            dy, dx = dirs[(d + turn) % 4]
            ny, nx = y + dy, x + dx
            if inside(ny, nx) and fg[ny, nx] and (not inside(ny + dy, nx + dx) or fg[ny + dy, nx + dx]):
                d, y, x = (d + turn) % 4, ny, nx
                fg[y, x] = False
                break
        else:
            break
    if not sealed:
        fg[0, 1] = False
    return fg


def _comb(H: int, W: int, closed: bool) -> np.ndarray:
    fg = np.zeros((H, W), bool)
    fg[1:2, 1:W - 1] = True
    fg[1:H - 1, 1:W - 1:2] = True
    if closed:  # a bar across the teeth ends: every slot becomes a hole
        fg[H - 2:H - 1, 1:W - 1] = True
    return fg


def _rings(H: int, W: int) -> np.ndarray:
    fg = np.zeros((H, W), bool)
    for k in range(1, min(H, W) // 2, 2):
        fg[k:H - k, k:W - k] = True
        fg[k + 1:H - k - 1, k + 1:W - k - 1] = False
    return fg


def _corner_opening(H: int, W: int) -> np.ndarray:
    """A cavity whose only way out is a corridor down column c that enters it at (c, c), the first
    pixel of a label tile (c = TILE where the image has one)."""
    fg = np.ones((H, W), bool)
    c = TILE if min(H, W) > TILE + 3 else min(H, W) // 2
    fg[c:H - 2, c:W - 2] = False
    fg[0:c, c:c + 1] = False
    return fg


def _labelling_cases(H: int, W: int) -> np.ndarray:
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([_spiral(H, W, False), _spiral(H, W, True), _comb(H, W, False), _comb(H, W, True),
                     (yy + xx) % 2 == 0, (yy + xx) % 2 == 1, _rings(H, W), np.ones((H, W), bool),
                     _corner_opening(H, W), ~_spiral(H, W, False), np.zeros((H, W), bool)])


@pytest.mark.parametrize("H,W", [(33, 47), (80, 144), (100, 131), (1, 1), (1, 17), (17, 1)])
def test_labelling_worst_cases(H, W):
    fg = _labelling_cases(H, W)
    want = _host_maps(fg)
    if H == 100:
        # the cases are what they claim: the open spiral's walls are outer contour all the way to
        # the centre, the sealed one has only the image border
        assert want[0][H // 2 - 2:H // 2 + 2].sum() > 0 and want[1].sum() == 2 * (H + W) - 4
        assert want[8][TILE:, TILE:].sum() > 0
    m = torch.from_numpy(fg.astype(np.float32))
    got = ev.extract_boundaries_device(m.cuda()).cpu().numpy()
    for i in range(len(fg)):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"case {i}")
    # as predictions against the reversed list as targets: sizes of the sets
    counts, bp, bt = _device(m * 0.75, torch.from_numpy(fg[::-1].astype(np.float32) * 0.3), 0.5, 2)
    np.testing.assert_array_equal(bp, want)
    np.testing.assert_array_equal(bt, want[::-1])
    np.testing.assert_array_equal(counts[:, 0], want.reshape(len(fg), -1).sum(1))
    np.testing.assert_array_equal(counts[:, 1], want[::-1].reshape(len(fg), -1).sum(1))


# ---------------------------------------------------------------------------- 3. random blobs

@functools.lru_cache(maxsize=None)
def _blobs(B: int, H: int, W: int, seed: int, sigma: float = 2.0):
    """Seeded Gaussian-filtered noise as probabilities in [0, 1] and a second field cut at its
    median as targets; sample 0 has an empty prediction, sample 1 an empty target."""
    rng = np.random.default_rng(seed)

    def field():
        f = np.stack([ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma) for _ in range(B)])
        return (f - f.min()) / (f.max() - f.min())
    p = field().astype(np.float32)
    t = (field() > 0.5).astype(np.float32)
    if B > 1:
        p[0] = 0.0
        t[1] = 0.0
    return torch.from_numpy(p), torch.from_numpy(t)


@pytest.mark.parametrize("H,W", [(48, 80), (33, 47)])
@pytest.mark.parametrize("thr", [0.4, 0.5, 0.6])
def test_random_blobs_exact(H, W, thr):
    p, t = _blobs(4, H, W, seed=11)
    hd = _check_exact(p, t, thr)
    assert np.isinf(hd[0]) and np.isinf(hd[1]) and np.isfinite(hd[2:]).all()
    counts = ev.boundary_counts(p.cuda(), t.cuda(), thr, 2).cpu().numpy()
    assert counts.dtype == np.int32 and counts.shape == (4, 6)
    assert (counts[:2, 2:4] == 0).all() and (counts[:2, 4:] == -1).all() and (counts[2:, 4:] >= 0).all()


# ---------------------------------------------------------------------------- 4. threshold semantics

def test_threshold_semantics():
    p = torch.full((1, 9, 9), 0.25)
    p[0, 2:7, 2:7] = 0.5         # == thr: background
    p[0, 3:6, 3:6] = 0.5000001   # the next float above: foreground
    p[0, 4, 4] = float("nan")    # background: a hole, so the contour is the 3 x 3 ring
    p[0, 0, 0] = float("nan")
    p[0, 8, 8] = float("inf")
    t = torch.zeros(1, 9, 9)
    t[0, 1:4, 1:4] = 0.3         # > 0: foreground
    t[0, 6, 6] = -1.0            # background
    want_p = np.zeros((9, 9), np.uint8)
    want_p[3:6, 3:6] = 1
    want_p[4, 4] = 0
    want_p[8, 8] = 1
    want_t = np.zeros((9, 9), np.uint8)
    want_t[1:4, 1:4] = 1
    want_t[2, 2] = 0
    counts, bp, bt = _device(p, t, 0.5, 2)
    np.testing.assert_array_equal(bp[0], want_p)
    np.testing.assert_array_equal(bt[0], want_t)
    assert counts[0, 0] == 9 and counts[0, 1] == 8
    np.testing.assert_array_equal(bp, _host_maps((p > 0.5).numpy()))
    np.testing.assert_array_equal(bt, _host_maps((t > 0).numpy()))


# ---------------------------------------------------------------------------- 5. scores

@pytest.mark.parametrize("tol", [0, 2, 3])
def test_scores_match_host(tol):
    p, t = _blobs(4, 48, 80, seed=11)
    want = ev.compute_boundary_f1_batch(p[:, None], t[:, None], 0.5, tol, backend="host")
    for kw in ({}, {"backend": "device"}, {"backend": "auto"}):
        got = ev.compute_boundary_f1_batch(p[:, None].cuda(), t[:, None].cuda(), 0.5, tol, **kw)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (4,)
        assert (got.cpu() - want).abs().max().item() <= 1e-6
    host = ev.compute_boundary_f1_batch(p[:, None].cuda(), t[:, None].cuda(), 0.5, tol, backend="host")
    assert not host.is_cuda and torch.equal(host, want)
    for i in (0, 2, 3):
        got = ev.compute_boundary_f1(p[i:i + 1, None].cuda(), t[i:i + 1, None].cuda(), 0.5, tol)
        assert abs(got.item() - want[i].item()) <= 1e-6


# ---------------------------------------------------------------------------- 6. determinism

def test_two_calls_are_bitwise_equal():
    p, t = _blobs(4, 48, 80, seed=11)
    pc, tc = p.cuda(), t.cuda()
    a = ev._boundary_device(pc, tc, 0.5, 2, maps=True)
    b = ev._boundary_device(pc, tc, 0.5, 2, maps=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    fg = torch.from_numpy(_labelling_cases(100, 131).astype(np.float32)).cuda()
    a = ev._boundary_device(fg, fg.flip(0), 0.5, 3, maps=True)
    b = ev._boundary_device(fg, fg.flip(0), 0.5, 3, maps=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------- 7. widths

@pytest.mark.parametrize("H,W,sigma", [(16, 4096, 2.0), (512, 512, 3.0)])
def test_wide_and_full_size_exact(H, W, sigma):
    p, t = _blobs(1, H, W, seed=5, sigma=sigma)
    hd = _check_exact(p, t, 0.5, tolerances=(0, 2, 5))
    assert np.isfinite(hd).all()


def test_far_apart_sets_in_a_wide_row():
    """One boundary pixel at each end of a 1 x 4096 row and of a 4096 x 1 column: the largest
    distance the uint16 column map and the int32 squares have to carry."""
    for shape in ((1, 1, 4096), (1, 4096, 1)):
        p, t = torch.zeros(shape), torch.zeros(shape)
        p.view(-1)[0] = 1.0
        t.view(-1)[-1] = 1.0
        counts = ev.boundary_counts(p.cuda(), t.cuda(), 0.5, 5).cpu().numpy()
        np.testing.assert_array_equal(counts, [[1, 1, 0, 0, 4095 * 4095, 4095 * 4095]])
        assert ev.compute_hausdorff_distance_batch(p.cuda(), t.cuda()).item() == 4095.0


def test_bad_shapes_are_argument_errors():
    with pytest.raises(ValueError):
        ev.boundary_counts(torch.zeros(1, 2, 4097, device="cuda"), torch.zeros(1, 2, 4097, device="cuda"))
    with pytest.raises(ValueError):
        ev.boundary_counts(torch.zeros(1, 8, 8, device="cuda"), torch.zeros(2, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        ev.compute_boundary_f1_batch(torch.zeros(1, 1, 8, 8, device="cuda"), torch.zeros(1, 1, 8, 8), backend="device")


# ---------------------------------------------------------------------------- 8. loops

def _two_models():
    from physics_informed_image_segmentation_amd import UNet
    torch.manual_seed(42)
    a = UNet(1, 1, 64, dropout=0.0).cuda()
    b = UNet(1, 1, 64, dropout=0.0).cuda()
    b.load_state_dict(a.state_dict())
    img, mask = rt.synthetic_batch(6, 64, 64, seed=7)
    return a, b, [(img[k:k + 2], mask[k:k + 2]) for k in (0, 2, 4)]


def _same_but_bf1(host, dev):
    assert set(host) == set(dev)
    for k, v in host.items():
        if k == "boundary_f1_score":
            assert dev[k] == pytest.approx(v, rel=1e-6), (dev[k], v)
            assert v > 0
        else:
            assert dev[k] == v, (k, dev[k], v)


def test_validate_and_train_epoch_backends_agree(hip):
    from physics_informed_image_segmentation_amd import AdamW, DiceBCEPDELoss
    tr = importlib.import_module("physics_informed_image_segmentation_amd.train")
    kw = dict(pde_weight=1e-2, phase_field_weight=1e-2, diffusion_coeff=5.0, reaction_threshold=0.5, epsilon=0.05)
    a, b, batches = _two_models()
    dev = torch.device("cuda")
    res = [tr.validate(m, batches, DiceBCEPDELoss(**kw), dev, return_components=True, boundary_backend=be)
           for m, be in ((a, "host"), (b, "device"))]
    _same_but_bf1(*res)
    auto = tr.validate(b, batches, DiceBCEPDELoss(**kw), dev, return_components=True)
    assert auto == res[1]  # "auto" on a CUDA device is the device scorer
    res = [tr.train_epoch(m, batches, DiceBCEPDELoss(**kw), AdamW(m.parameters(), lr=1e-4, weight_decay=1e-5), dev,
                          return_components=True, boundary_backend=be)
           for m, be in ((a, "host"), (b, "device"))]
    _same_but_bf1(*res)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


# ---------------------------------------------------------------------------- 9. evaluate_model

def test_evaluate_model_backends_agree(hip):
    a, _, batches = _two_models()
    # an empty prediction and an empty target: NaN Hausdorff entries in the same places
    img, mask = batches[1][0].clone(), batches[1][1].clone()
    mask[1] = 0.0
    loader = [batches[0], (img, mask)]
    dev = torch.device("cuda")
    host = ev.evaluate_model(a, loader, dev, boundary_backend="host")
    for be in ("device", "auto"):
        got = ev.evaluate_model(a, loader, dev, boundary_backend=be)
        assert set(got) == set(host) == {"dice_scores", "iou_scores", "boundary_f1_scores", "hausdorff_distances"}
        np.testing.assert_array_equal(got["dice_scores"], host["dice_scores"])
        np.testing.assert_array_equal(got["iou_scores"], host["iou_scores"])
        assert got["boundary_f1_scores"].shape == (4,)
        assert np.abs(got["boundary_f1_scores"] - host["boundary_f1_scores"]).max() <= 1e-6
        np.testing.assert_array_equal(got["hausdorff_distances"], host["hausdorff_distances"])
        assert np.isnan(got["hausdorff_distances"][3])
