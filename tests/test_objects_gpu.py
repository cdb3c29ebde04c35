"""Object-level metrics on the device (csrc/components.hip through evaluate.py) against the host
path of evaluate.py (scipy.ndimage.label + numpy) on .cpu() copies. Everything is integer
geometry: counters and label maps are compared with ==, for connectivity 4 and 8.

The label kernel's tile is 32 x 32: the shapes run from 1 x 1 over one tile plus a remainder
(33 x 47) to 100 x 131 (three tiles plus a remainder down, four plus a remainder across)."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

from oracle import reference_torch as rt
from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd import evaluate as ev

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 70), (70, 1), (31, 33), (33, 47), (64, 96), (100, 131)]


def _device(p, t, thr, conn, min_area, **kw):
    counts, lp, lt = ev._objects_device(p.cuda(), t.cuda(), thr, conn, min_area, maps=True, **kw)
    assert counts.dtype == torch.int64 and lp.dtype == torch.int32 and lt.dtype == torch.int32
    return counts.cpu().numpy(), lp.cpu().numpy(), lt.cpu().numpy()


def _check(p, t, thr=0.5, conns=(4, 8), min_areas=(0,)):
    """Counters and both label maps of a (B, H, W) pair, device == host; returns the host counters
    of the last combination."""
    p, t = torch.as_tensor(p, dtype=torch.float32), torch.as_tensor(t, dtype=torch.float32)
    for conn in conns:
        for ma in min_areas:
            want = ev._objects_host(p, t, thr, conn, ma)
            got = _device(p, t, thr, conn, ma)
            for g, w, what in zip(got, want, ("counts", "labels_p", "labels_t")):
                np.testing.assert_array_equal(g, w, err_msg=f"{what}, connectivity {conn}, min_area {ma}")
            # without the label maps (fewer launches): the same counters
            only = ev.object_counts(p.cuda(), t.cuda(), thr, conn, ma)
            assert only.is_cuda and only.dtype == torch.int64
            np.testing.assert_array_equal(only.cpu().numpy(), want[0])
    return want[0]


@functools.lru_cache(maxsize=None)
def _noise(B, H, W, seed, sigma=1.5):
    """Seeded Gaussian-filtered noise as probabilities in [0, 1] and a second field cut at its
    middle as targets."""
    rng = np.random.default_rng(seed)

    def field():
        f = np.stack([ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma) for _ in range(B)])
        return (f - f.min()) / max(f.max() - f.min(), 1e-30)
    return torch.from_numpy(field().astype(np.float32)), torch.from_numpy((field() > 0.5).astype(np.float32))


# ---------------------------------------------------------------------------- the hand-computed cases

def _case_a():
    t, p = np.zeros((6, 8), np.float32), np.zeros((6, 8), np.float32)
    t[1:3, 1:3] = 1
    t[4, 4:8] = 1
    p[1:3, 1] = 1
    p[4, 5:8] = 1
    p[0, 7] = 1
    return p, t


def _checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2).astype(np.float32)


def _counts(p, t, conn=8, min_area=0):
    return ev.object_counts(torch.from_numpy(p)[None].cuda(), torch.from_numpy(t)[None].cuda(), 0.5, conn,
                            min_area).cpu()[0].tolist()


def test_case_a():
    p, t = _case_a()
    assert _counts(p, t) == [3, 2, 1, 0, 5, 9, 6, 0]
    assert _counts(p, t, min_area=2) == [2, 2, 1, 0, 5, 8, 5, 1]
    _check(p[None], t[None], min_areas=(0, 2))


def test_case_b():
    t, p = np.zeros((6, 8), np.float32), np.zeros((6, 8), np.float32)
    t[2, 0:3] = 1
    t[2, 4:8] = 1
    p[2, 1:7] = 1
    assert _counts(p, t) == [1, 2, 0, 0, 5, 14, 6, 0]
    _check(p[None], t[None])


def test_case_c():
    m = np.zeros((64, 64), np.float32)
    for y, x in ((31, 31), (32, 32), (31, 40), (32, 39)):
        m[y, x] = 1
    assert _counts(m, m, 8) == [2, 2, 2, 2, 4, 4, 4, 0]
    assert _counts(m, m, 4) == [4, 4, 4, 4, 4, 4, 4, 0]
    _check(m[None], m[None])


def test_case_d():
    cb = _checkerboard(33, 47)
    assert _counts(cb, cb, 4) == [775] * 7 + [0]
    assert _counts(cb, cb, 8) == [1, 1, 1, 1, 775, 775, 775, 0]
    assert _counts(cb, 1 - cb, 8) == [1, 1, 0, 0, 0, 1551, 775, 0]
    _check(np.stack([cb, cb]), np.stack([cb, 1 - cb]))


# ---------------------------------------------------------------------------- shapes, batches, noise

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_noise_exact(H, W, B):
    for seed in (3, 4, 5):
        p, t = _noise(B, H, W, seed)
        c = _check(p, t)
        if H * W >= 31 * 33:
            assert c[:, :2].min() >= 1  # there are objects to match


@pytest.mark.parametrize("H,W", SHAPES)
def test_full_and_single_pixel_images(H, W):
    one = np.zeros((H, W), np.float32)
    one[H - 1, W - 1] = 1
    full = np.ones((H, W), np.float32)
    c = _check(np.stack([full, one, full]), np.stack([full, full, one]))
    np.testing.assert_array_equal(c[0], [1, 1, 1, 1, H * W, H * W, H * W, 0])


# ---------------------------------------------------------------------------- labelling worst cases

def _spiral(H, W):
    """A one-pixel path spiralling inwards from (0, 0) with one pixel of background between its
    turns: one object under both connectivities, crossing every tile edge many times."""
    fg = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    fg[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ahead = 0 <= ay < H and 0 <= ax < W and fg[ay, ax]
        if 0 <= ny < H and 0 <= nx < W and not fg[ny, nx] and not ahead:
            y, x, turns = ny, nx, 0
            fg[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return fg


def _comb(H, W):
    fg = np.zeros((H, W), bool)
    fg[1, 1:W - 1] = True
    fg[1:H - 1, 1:W - 1:2] = True
    return fg


def _frame(H, W):
    fg = np.zeros((H, W), bool)
    fg[[0, H - 1], :] = True
    fg[:, [0, W - 1]] = True
    return fg


def _corner_diagonals(H, W):
    """Two pixels that touch only diagonally, across four-tile corners: the main diagonal at
    (32, 32) and (64, 96), the anti-diagonal at (32, 64) and (64, 32)."""
    fg = np.zeros((H, W), bool)
    for y, x in ((32, 32), (64, 96)):
        fg[y - 1, x - 1] = fg[y, x] = True
    for y, x in ((32, 64), (64, 32)):
        fg[y - 1, x] = fg[y, x - 1] = True
    return fg


def test_labelling_worst_cases():
    H, W = 100, 131
    cases = np.stack([_spiral(H, W), _comb(H, W), _frame(H, W), _corner_diagonals(H, W), ~_spiral(H, W),
                      _comb(W, H).T]).astype(np.float32)
    # the cases are what they claim: the spiral and the frame are one object each, and the corner
    # diagonals join under 8-connectivity only
    n4 = ev._objects_host(torch.from_numpy(cases), torch.from_numpy(cases), 0.5, 4, 0)[0][:, 0]
    n8 = ev._objects_host(torch.from_numpy(cases), torch.from_numpy(cases), 0.5, 8, 0)[0][:, 0]
    assert n4[0] == n8[0] == 1 and n4[1] == 1 and n4[2] == n8[2] == 1
    assert n4[3] == 8 and n8[3] == 4
    p = torch.from_numpy(cases)
    _check(p, p)
    _check(p * 0.75, p.flip(0) * 0.3)          # each against another one: many pairs per object
    _check(p, torch.from_numpy(_checkerboard(H, W))[None].expand(len(cases), H, W))


def test_checkerboard_fills_the_pair_table():
    """The same 100 x 131 checkerboard as prediction and target at 4-connectivity: every
    foreground pixel is an object and a pair of its own, the most distinct pairs an image of this
    size can have. The table holds them all: no counter is -1."""
    cb = _checkerboard(100, 131)
    c = _check(np.stack([cb, 1 - cb]), np.stack([cb, 1 - cb]), conns=(4,))
    assert (c >= 0).all() and c[0].tolist() == [6550] * 7 + [0]
    got = ev.object_counts(torch.from_numpy(cb)[None].cuda(), torch.from_numpy(cb)[None].cuda(), 0.5, 4)
    assert got.cpu()[0].tolist() == [6550] * 7 + [0]


def test_nan_prediction():
    p, t = _noise(3, 64, 96, 7)
    p = p.clone()
    p[0, ::5, ::3] = float("nan")
    p[1, 30:34] = float("nan")  # a NaN band across a tile edge cuts objects apart
    p[2] = float("nan")
    c = _check(p, t)
    assert c[2, 0] == 0 and c[2, 1] > 0


# ---------------------------------------------------------------------------- min_area

def test_min_area():
    p, t = _noise(3, 100, 131, 9, sigma=1.0)
    areas = np.concatenate([np.bincount(lab.ravel())[1:] for lab in ev._objects_host(p, t, 0.5, 8, 0)[1]])
    assert (areas < 5).any() and (areas >= 5).any()  # 5 removes some objects and keeps some
    huge = int(areas.max()) + 1
    seen = {}
    for ma in (0, 1, 5, huge):
        seen[ma] = _check(p, t, min_areas=(ma,))
    np.testing.assert_array_equal(seen[0], seen[1])
    assert seen[5][:, 7].sum() > 0 and (seen[5][:, 0] + seen[5][:, 7] == seen[0][:, 0]).all()
    # removed objects leave the pairs and the AJI union: with everything removed the union is
    # the targets' area alone
    t_area = (t > 0).reshape(3, -1).sum(1).numpy()
    np.testing.assert_array_equal(seen[huge][:, [0, 2, 3, 4, 6]], 0)
    np.testing.assert_array_equal(seen[huge][:, 5], t_area)
    np.testing.assert_array_equal(seen[huge][:, 7], seen[0][:, 0])


# ---------------------------------------------------------------------------- batches and repeats

def test_samples_do_not_leak():
    p, t = _noise(1, 100, 131, 3)
    zero, one = torch.zeros_like(p), torch.ones_like(p)
    alone = _check(p, t)
    c = _check(torch.cat([zero, one, p]), torch.cat([zero, one, t]))
    np.testing.assert_array_equal(c[0], [0] * 8)
    np.testing.assert_array_equal(c[1], [1, 1, 1, 1, 13100, 13100, 13100, 0])
    np.testing.assert_array_equal(c[2], alone[0])


def test_two_calls_are_bitwise_equal_and_the_workspace_holds_no_state():
    p, t = _noise(3, 100, 131, 4)
    pc, tc = p.cuda(), t.cuda()
    for conn, ma in ((8, 0), (4, 3)):
        a = ev._objects_device(pc, tc, 0.5, conn, ma, maps=True)
        b = ev._objects_device(pc, tc, 0.5, conn, ma, maps=True)
        ws = torch.full((_hip.lib().pis_objects_ws(3, 100, 131),), 0xFF, dtype=torch.uint8, device="cuda")
        c = ev._objects_device(pc, tc, 0.5, conn, ma, maps=True, ws=ws)
        # the same workspace again, now holding the previous call's leftovers
        d = ev._objects_device(tc, pc, 0.5, conn, ma, maps=True, ws=ws)
        e = ev._objects_device(pc, tc, 0.5, conn, ma, maps=True, ws=ws)
        for x, y, z, w in zip(a, b, c, e):
            assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w)
        assert not torch.equal(d[0], a[0])


# ---------------------------------------------------------------------------- Python surface

def test_label_components():
    p, _ = _noise(3, 100, 131, 5)
    for conn in (4, 8):
        for ma in (0, 4):
            want_l, want_n = ev.label_components(p, 0.5, conn, ma)
            for kw in ({}, {"backend": "device"}):
                lab, n = ev.label_components(p.cuda(), 0.5, conn, ma, **kw)
                assert lab.is_cuda and lab.dtype == torch.int32 and lab.shape == (3, 100, 131)
                assert n.is_cuda and n.dtype == torch.int64 and n.shape == (3,)
                assert torch.equal(lab.cpu(), want_l) and torch.equal(n.cpu(), want_n)
            assert int(lab.max()) == int(n.max())
    lab, n = ev.label_components(p.cuda(), 0.5, backend="host")
    assert not lab.is_cuda and torch.equal(lab, ev.label_components(p, 0.5)[0])
    # default threshold 0: a mask; (B, 1, H, W) input
    m = (p > 0.5).float()
    assert torch.equal(ev.label_components(m[:, None].cuda())[0].cpu(), ev.label_components(p, 0.5)[0])


def test_scores_match_host():
    p, t = _noise(3, 64, 96, 6)
    p, t = torch.cat([p, torch.zeros(1, 64, 96)]), torch.cat([t, torch.zeros(1, 64, 96)])
    for fn, kws in ((ev.compute_object_f1_batch, ({}, {"iou": 0.75}, {"connectivity": 4, "min_area": 3})),
                    (ev.compute_aji_batch, ({}, {"connectivity": 4, "min_area": 3}))):
        for kw in kws:
            want = fn(p, t, **kw)
            got = fn(p[:, None].cuda(), t[:, None].cuda(), **kw)
            assert got.is_cuda and got.dtype == torch.float64 and got.shape == (4,)
            np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
            assert np.isnan(want[3].item()) and np.isfinite(want[:3].numpy()).all()
    host = ev.object_counts(p.cuda(), t.cuda(), backend="host")
    assert not host.is_cuda and torch.equal(host, ev.object_counts(p, t))


def test_bad_arguments():
    z = torch.zeros(1, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        ev.object_counts(torch.zeros(1, 2, 4097, device="cuda"), torch.zeros(1, 2, 4097, device="cuda"))
    with pytest.raises(ValueError):
        ev.object_counts(z, torch.zeros(2, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        ev.object_counts(z, torch.zeros(1, 8, 8), backend="device")
    for kw in (dict(connectivity=6), dict(min_area=-1), dict(backend="gpu")):
        with pytest.raises(ValueError):
            ev.object_counts(z, z, **kw)


# ---------------------------------------------------------------------------- C ABI errors

def test_capi_errors(hip):
    z = torch.zeros(1, 16, 16, device="cuda")
    counts = torch.zeros(1, 8, dtype=torch.int64, device="cuda")
    need = hip.pis_objects_ws(1, 16, 16)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = _hip.stream_handle(z.device)

    def call(B=1, H=16, W=16, conn=8, min_area=0, ws_bytes=need):
        rc = hip.pis_object_metrics(z.data_ptr(), z.data_ptr(), B, H, W, ctypes.c_float(0.5), conn, min_area,
                                    counts.data_ptr(), 0, 0, ws.data_ptr(), ws_bytes, stream)
        return rc, hip.pis_last_error()

    for kw in (dict(B=0), dict(H=0), dict(W=4097), dict(H=4097), dict(conn=6), dict(conn=1), dict(min_area=-1)):
        rc, msg = call(**kw)
        assert rc == -1 and b"pis_object_metrics" in msg, kw
    rc, msg = call(ws_bytes=need - 1)
    assert rc == -3 and b"workspace" in msg
    assert hip.pis_objects_ws(1, 4097, 4) == 0 and hip.pis_objects_ws(1, 4, 4097) == 0
    assert hip.pis_objects_ws(1, 4096, 4096) > 0
    assert call()[0] == 0  # the valid call goes through
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [[0] * 8]


# ---------------------------------------------------------------------------- evaluate_model, CLI

BASE_KEYS = {"dice_scores", "iou_scores", "boundary_f1_scores", "hausdorff_distances"}
OBJECT_KEYS = {"object_f1_scores", "aji_scores", "object_count_errors"}


def test_evaluate_model_object_metrics(hip):
    from physics_informed_image_segmentation_amd import UNet
    torch.manual_seed(42)
    net = UNet(1, 1, 64, dropout=0.0).cuda()
    img, mask = rt.synthetic_batch(4, 64, 64, seed=7)
    mask = mask.clone()
    mask[3] = 0.0
    loader = [(img[:2], mask[:2]), (img[2:], mask[2:])]
    dev = torch.device("cuda")
    off = ev.evaluate_model(net, loader, dev)
    assert set(off) == BASE_KEYS
    host = ev.evaluate_model(net, loader, dev, object_metrics=True, object_backend="host")
    for kw in ({}, {"object_backend": "device"}):
        got = ev.evaluate_model(net, loader, dev, object_metrics=True, **kw)
        assert set(got) == set(host) == BASE_KEYS | OBJECT_KEYS
        for k in BASE_KEYS | OBJECT_KEYS:
            assert got[k].shape == (4,) and got[k].dtype == np.float64
            np.testing.assert_array_equal(got[k], host[k], err_msg=k)
        for k in BASE_KEYS:
            np.testing.assert_array_equal(got[k], off[k], err_msg=k)
    # the arrays are what the batch functions give
    net.eval()
    with torch.no_grad():
        out = torch.cat([net(x.cuda()) for x, _ in loader])
    np.testing.assert_array_equal(host["aji_scores"], ev.compute_aji_batch(out.cpu(), mask).numpy())
    np.testing.assert_array_equal(host["object_f1_scores"], ev.compute_object_f1_batch(out.cpu(), mask).numpy())
    c = ev.object_counts(out.cpu(), mask)
    np.testing.assert_array_equal(host["object_count_errors"], (c[:, 0] - c[:, 1]).numpy())
    got4 = ev.evaluate_model(net, loader, dev, boundary_metrics=False, object_metrics=True, connectivity=4,
                             min_object_area=3)
    assert set(got4) == {"dice_scores", "iou_scores"} | OBJECT_KEYS
    c4 = ev.object_counts(out.cpu(), mask, 0.5, 4, 3)
    np.testing.assert_array_equal(got4["object_count_errors"], (c4[:, 0] - c4[:, 1]).numpy())
    with pytest.raises(ValueError):
        ev.evaluate_model(net, loader, dev, object_metrics=True, connectivity=5)


def _coco_folder(tmp_path, n=3, H=64, W=64):
    d = tmp_path / "testing"
    d.mkdir()
    imgs, anns = [], []
    for i in range(n):
        a = np.full((H, W), 40, np.uint8)
        x0, y0 = 8 + 6 * i, 10 + 4 * i
        a[y0:y0 + 20, x0:x0 + 24] = 200
        Image.fromarray(a, mode="L").save(d / f"{i}.png")
        imgs.append({"id": i, "file_name": f"{i}.png", "height": H, "width": W})
        anns.append({"id": 100 + i, "image_id": i,
                     "segmentation": [[x0, y0, x0 + 23, y0, x0 + 23, y0 + 19, x0, y0 + 19]]})
    js = tmp_path / "test.json"
    js.write_text(json.dumps({"images": imgs, "annotations": anns}))
    return d, js


def test_eval_cli_object_metrics(hip, tmp_path):
    import evaluate as eval_cli
    from physics_informed_image_segmentation_amd import UNet
    d, js = _coco_folder(tmp_path)
    paths = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        p = tmp_path / f"m{seed}.pth"
        torch.save(UNet(1, 1, 64).state_dict(), p)
        paths.append(p)
    out = tmp_path / "out"
    common = ["--baseline", str(paths[0]), "--pde", str(paths[1]), "--test-dir", str(d), "--test-json", str(js),
              "--batch-size", "2", "--output-dir", str(out)]
    base_header = ["image_id", "baseline_dice", "pde_dice", "baseline_iou", "pde_iou", "baseline_boundary_f1",
                   "pde_boundary_f1", "baseline_hausdorff", "pde_hausdorff"]
    # (the device-resident cache serves the same batches without starting loader workers)
    res = eval_cli.main(common + ["--device-cache", "--object-metrics", "--connectivity", "4",
                                  "--min-object-area", "2"])
    assert set(res["baseline_metrics"]) == set(res["pde_metrics"]) == BASE_KEYS | OBJECT_KEYS
    assert len(res["baseline_metrics"]["aji_scores"]) == 3
    header = open(res["results_csv"]).readline().strip().split(",")
    assert header == base_header + ["baseline_object_f1", "pde_object_f1", "baseline_aji", "pde_aji",
                                    "baseline_object_count_error", "pde_object_count_error"]
    assert set(json.load(open(res["comparison_json"]))) == BASE_KEYS | OBJECT_KEYS
    summary = [line.split(",")[0] for line in open(res["summary_csv"]).read().splitlines()[1:]]
    assert summary == ["dice_scores", "iou_scores", "boundary_f1_scores", "hausdorff_distances", "object_f1_scores",
                       "aji_scores", "object_count_errors"]
    # without the switch: today's keys and columns
    res = eval_cli.main(common)
    assert set(res["baseline_metrics"]) == BASE_KEYS
    assert open(res["results_csv"]).readline().strip().split(",") == base_header
    assert set(json.load(open(res["comparison_json"]))) == BASE_KEYS
