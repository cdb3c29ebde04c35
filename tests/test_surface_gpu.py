"""Distance transform and surface distances on the device (csrc/distance.hip through evaluate.py)
against the host definitions of record on .cpu() copies. The tables are integer geometry and are
compared with ==, against scipy's transform and, independently, against the counters of
pis_boundary_metrics; the percentile Hausdorff distance is the square root of an integer both
backends select with ==, the surface Dice one division of equal integers, and the ASSD a float64
sum of non-negative terms whose order differs between the backends (n 2^-52 relative).

Shapes: the column pass works in 32-row segments and the row pass in 64-column blocks, so the cases
run below, at and across both (1, 33, 65, 70, 130, 257, 300), on the longest strips either way (the
largest distance, 4095^2) and, for the pruned outward search, at 512 x 512 with one set pixel."""
import functools
import json

import numpy as np
import pytest
import torch
from scipy import ndimage

from oracle import reference_torch as rt
from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd import evaluate as ev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (2, 33, 65), (3, 70, 130), (1, 257, 300), (1, 3, 4096), (1, 4096, 3)]


def _sets(N, H, W, seed=5):
    """name -> (N, H, W) bool: empty, full, one pixel in each corner, one full row, one full column,
    seeded random at two densities (other rows / columns / pixels in every image of the batch)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    z = np.zeros((N, H, W), bool)
    out = {"empty": z, "full": ~z}
    for name, (y, x) in (("tl", (0, 0)), ("tr", (0, W - 1)), ("bl", (H - 1, 0)), ("br", (H - 1, W - 1))):
        m = z.copy()
        m[:, y, x] = True
        out[name] = m
    row, col = z.copy(), z.copy()
    for i in range(N):
        row[i, (H // 3 + 7 * i) % H, :] = True
        col[i, :, (2 * W // 3 + 11 * i) % W] = True
    out["row"], out["col"] = row, col
    out["sparse"] = rng.random((N, H, W)) < 0.001
    out["dense"] = rng.random((N, H, W)) < 0.5
    return out


def _check_transform(m: np.ndarray, name=""):
    want = ev.distance_transform_sq_np(m)
    got = ev.distance_transform_sq(torch.from_numpy(m.astype(np.float32)).cuda())
    assert got.dtype == torch.int32 and got.is_cuda and got.shape == m.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=name)
    return want


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_transform_equals_host(hip, N, H, W):
    for name, m in _sets(N, H, W).items():
        want = _check_transform(m, name)
        if name == "tl":      # the far end of the image: the largest distance there is
            assert want[0, -1, -1] == (H - 1) ** 2 + (W - 1) ** 2


def test_transform_worst_case_search_and_mixed_batch(hip):
    # one set pixel: every other pixel's search crosses the row through empty 64-column blocks
    for name, m in _sets(1, 512, 512).items():
        if name in ("tl", "tr", "bl", "br", "sparse"):
            _check_transform(m, name)
    # an empty, a full and a random image side by side: EDT_NONE is per image
    s = _sets(1, 70, 130)
    want = _check_transform(np.concatenate([s["empty"], s["full"], s["sparse"], s["empty"], s["dense"]]))
    assert (want[0] == ev.EDT_NONE).all() and (want[1] == 0).all() and (want[3] == ev.EDT_NONE).all()
    assert 0 < want[2].max() < ev.EDT_NONE
    # input forms: (B, 1, H, W), (H, W), values that are not 0 / 1, NaN outside the set
    x = torch.from_numpy(s["dense"].astype(np.float32)) * 3.5
    x[0, 0, :5] = float("nan")
    x[0, 1, :5] = -1.0
    want = ev.distance_transform_sq_np(x.numpy())
    for form in (x, x[:, None], x[0]):
        np.testing.assert_array_equal(ev.distance_transform_sq(form.cuda()).cpu().numpy(), want)
    assert not ev.distance_transform_sq(x.cuda(), backend="host").is_cuda
    with pytest.raises(ValueError):
        ev.distance_transform_sq(torch.zeros(1, 2, 4097, device="cuda"))


def test_every_pruning_of_the_row_pass_gives_the_same_integers(hip):
    """pis_tune key PIS_TUNE_EDT_PRUNE: 0 plain outward search, 1 blocks skipped, 3 (shipped) steps too."""
    cases = [_sets(1, 257, 300)[k] for k in ("tl", "br", "row", "col", "sparse", "dense", "empty")]
    cases += [_sets(1, 512, 512)[k] for k in ("tr", "sparse")] + [_sets(1, 3, 4096)["tl"], _sets(1, 4096, 3)["br"]]
    want = [ev.distance_transform_sq_np(m) for m in cases]
    p, t, want_pt, want_tp = _case(3, 70, 130)
    assert hip.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, -1) == 3
    for v in (0, 1, 3):
        prev = hip.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, v)
        try:
            for m, w in zip(cases, want):
                got = ev.distance_transform_sq(torch.from_numpy(m.astype(np.float32)).cuda())
                np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=f"key 55 = {v}, {m.shape}")
            got_pt, got_tp = ev.surface_distances(p.cuda(), t.cuda(), 0.5)
            assert torch.equal(got_pt.cpu(), want_pt) and torch.equal(got_tp.cpu(), want_tp)
        finally:
            hip.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, prev)
    assert hip.pis_tune(_hip.PIS_TUNE_EDT_PRUNE, -1) == 3


# ---------------------------------------------------------------------------- surface distances

@functools.lru_cache(maxsize=None)
def _case(B: int, H: int, W: int):
    """Blurred-noise predictions against disc (even samples) and blob (odd samples) targets, seeded;
    from B = 3 on sample 1 has an empty target, from B = 8 on sample 0 an empty prediction. Returns
    (p, t, host d2_pt, host d2_tp)."""
    rng = np.random.default_rng(100 * B + H)

    def field(sigma):
        f = np.stack([ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma) for _ in range(B)])
        return (f - f.min()) / (f.max() - f.min())
    p = field(2.0).astype(np.float32)
    t = (field(3.0) > 0.5).astype(np.float32)
    yy, xx = np.mgrid[:H, :W]
    for i in range(0, B, 2):
        cy, cx, r = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.15, 0.35) * min(H, W)
        t[i] = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.float32)
        p[i] = np.clip(0.6 * t[i] + 0.6 * p[i], 0, 1)          # a noisy copy of the disc
    if B >= 3:
        t[1] = 0.0
    if B >= 8:
        p[0] = 0.0
    p, t = torch.from_numpy(p), torch.from_numpy(t)
    d2_pt, d2_tp = ev.surface_distances(p, t, 0.5, backend="host")
    return p, t, d2_pt, d2_tp


CASES = [(2, 33, 65), (3, 70, 130), (8, 128, 128)]


@pytest.mark.parametrize("B,H,W", CASES)
def test_surface_distances_equal_host(hip, B, H, W):
    p, t, want_pt, want_tp = _case(B, H, W)
    got_pt, got_tp = ev.surface_distances(p.cuda(), t.cuda(), 0.5)
    assert got_pt.is_cuda and got_pt.dtype == got_tp.dtype == torch.int32 and got_pt.shape == got_tp.shape == (B, H, W)
    assert torch.equal(got_pt.cpu(), want_pt) and torch.equal(got_tp.cpu(), want_tp)
    n_p, n_t = (want_pt >= 0).sum((1, 2)), (want_tp >= 0).sum((1, 2))
    if B >= 3:    # the boundary pixels opposite an empty boundary hold EDT_NONE
        assert n_t[1] == 0 and n_p[1] > 0 and (got_pt[1][got_pt[1] >= 0] == ev.EDT_NONE).all()
    if B >= 8:
        assert n_p[0] == 0 and n_t[0] > 0 and (got_tp[0][got_tp[0] >= 0] == ev.EDT_NONE).all()
    assert ((n_p > 0) & (n_t > 0)).sum() >= 2
    # (B, 1, H, W) inputs, another threshold, the host path of CUDA tensors
    a, b = ev.surface_distances(p[:, None].cuda(), t[:, None].cuda(), 0.4)
    ha, hb = ev.surface_distances(p.cuda(), t.cuda(), 0.4, backend="host")
    assert not ha.is_cuda and torch.equal(a.cpu(), ha) and torch.equal(b.cpu(), hb)


@pytest.mark.parametrize("B,H,W", CASES)
def test_tables_agree_with_the_boundary_counters(hip, B, H, W):
    """Independent of scipy: n, m and the directed squared Hausdorff distances of pis_boundary_metrics."""
    p, t, _, _ = _case(B, H, W)
    pc, tc = p.cuda(), t.cuda()
    d2_pt, d2_tp = (x.reshape(B, -1) for x in ev.surface_distances(pc, tc, 0.5))
    for tol in (0, 2, 5):
        counts = ev.boundary_counts(pc, tc, 0.5, tol).cpu().numpy().astype(np.int64)
        n = torch.stack([(d2_pt >= 0).sum(1), (d2_tp >= 0).sum(1)], 1).cpu().numpy()
        m = torch.stack([((d2_pt >= 0) & (d2_pt <= tol * tol)).sum(1),
                         ((d2_tp >= 0) & (d2_tp <= tol * tol)).sum(1)], 1).cpu().numpy()
        h2 = torch.stack([d2_pt.max(1)[0], d2_tp.max(1)[0]], 1).cpu().numpy()
        np.testing.assert_array_equal(n, counts[:, 0:2])
        np.testing.assert_array_equal(m, counts[:, 2:4])
        both = (counts[:, 0] > 0) & (counts[:, 1] > 0)
        np.testing.assert_array_equal(h2[both], counts[both, 4:6])


@pytest.mark.parametrize("B,H,W", CASES)
def test_scores_device_against_host(hip, B, H, W):
    p, t, host_pt, host_tp = _case(B, H, W)
    dev = ev.surface_distances(p.cuda(), t.cuda(), 0.5)
    host = (host_pt, host_tp)
    for q in (1, 50, 95, 100):
        for d, h in zip(dev, host):      # the selected integers
            dn, dk = ev._percentile_d2(d.reshape(B, -1), q)
            hn, hk = ev._percentile_d2(h.reshape(B, -1), q)
            assert torch.equal(dn.cpu(), hn) and torch.equal(dk.cpu(), hk)
        got = ev.compute_hausdorff_percentile_batch(dev, percentile=q)
        want = ev.compute_hausdorff_percentile_batch(host, percentile=q)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (B,)
        assert torch.equal(got.cpu(), want), (q, got, want)
    hd = ev.compute_hausdorff_distance_batch(p.cuda(), t.cuda(), 0.5)
    assert torch.equal(ev.compute_hausdorff_percentile_batch(dev, percentile=100), hd)
    n = ((host_pt >= 0).sum((1, 2)) + (host_tp >= 0).sum((1, 2))).to(torch.float64)
    for tol in (0, 2, 5):
        got = ev.compute_surface_dice_batch(dev, tolerance=tol).cpu()
        want = ev.compute_surface_dice_batch(host, tolerance=tol)
        print("surface dice", tol, (got - want).abs().max().item())
        assert ((got - want).abs() <= 1e-15 * want.abs()).all()
    got, want = ev.compute_assd_batch(dev).cpu(), ev.compute_assd_batch(host)
    fin = torch.isfinite(want)
    print("assd", ((got - want).abs() / want.clamp_min(1e-300))[fin].max().item(), "bound",
          (n * 2.0 ** -52)[fin].min().item())
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and fin.sum() >= 2
    assert ((got - want).abs()[fin] <= (n * 2.0 ** -52 * want)[fin]).all()
    # predictions and targets in place of the pair: the same values, on the inputs' device
    assert torch.equal(ev.compute_assd_batch(p.cuda(), t.cuda()), ev.compute_assd_batch(dev))
    assert torch.equal(ev.compute_hausdorff_percentile_batch(p.cuda(), t.cuda(), backend="host"),
                       ev.compute_hausdorff_percentile_batch(host))


def test_two_calls_are_bitwise_equal(hip):
    p, t, _, _ = _case(8, 128, 128)
    pc, tc = p.cuda(), t.cuda()
    a, b = ev.surface_distances(pc, tc), ev.surface_distances(pc, tc)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    m = torch.from_numpy(_sets(3, 70, 130)["sparse"].astype(np.float32)).cuda()
    assert torch.equal(ev.distance_transform_sq(m), ev.distance_transform_sq(m))


# ---------------------------------------------------------------------------- evaluate_model, CLI

@functools.lru_cache(maxsize=None)
def _net():
    from physics_informed_image_segmentation_amd import UNet
    torch.manual_seed(42)
    return UNet(1, 1, 64, dropout=0.0).cuda().eval()


def test_evaluate_model_surface_metrics(hip):
    net = _net()
    img, mask = rt.synthetic_batch(4, 64, 64, seed=7)
    mask = mask.clone()
    mask[3] = 0.0                         # an empty target: NaN, as hausdorff_distances
    loader = [(img[:2], mask[:2]), (img[2:], mask[2:])]
    dev = torch.device("cuda")
    base = ev.evaluate_model(net, loader, dev)
    assert list(base) == ["dice_scores", "iou_scores", "boundary_f1_scores", "hausdorff_distances"]
    off = ev.evaluate_model(net, loader, dev, surface_metrics=False, surface_percentile=50, surface_tolerance=7)
    assert list(off) == list(base)
    for k in base:
        np.testing.assert_array_equal(off[k], base[k], err_msg=k)
    got = ev.evaluate_model(net, loader, dev, surface_metrics=True, surface_percentile=90, surface_tolerance=3)
    assert list(got) == list(base) + list(ev.SURFACE_METRIC_KEYS)
    for k in base:
        np.testing.assert_array_equal(got[k], base[k], err_msg=k)
    hdp, assd, dice = [], [], []
    with torch.no_grad():
        for x, m in loader:
            u, m = net(x.cuda()), m.cuda()
            hdp.extend(ev.compute_hausdorff_percentile_batch(u, m, percentile=90).tolist())
            assd.extend(ev.compute_assd_batch(u, m).tolist())
            dice.extend(ev.compute_surface_dice_batch(u, m, tolerance=3).tolist())
    assert np.isinf(hdp[3]) and np.isinf(assd[3])
    hdp, assd = (np.where(np.isfinite(v), v, np.nan) for v in (np.array(hdp), np.array(assd)))
    np.testing.assert_array_equal(np.isnan(hdp), np.isnan(base["hausdorff_distances"]))
    np.testing.assert_array_equal(got["hausdorff_percentile_distances"], np.array(hdp))
    np.testing.assert_array_equal(got["assd_distances"], np.array(assd))
    np.testing.assert_array_equal(got["surface_dice_scores"], np.array(dice))
    assert all(v.dtype == np.float64 and v.shape == (4,) for v in (got[k] for k in ev.SURFACE_METRIC_KEYS))
    # percentile 100 is the Hausdorff column; the host backend gives the same integers
    full = ev.evaluate_model(net, loader, dev, surface_metrics=True, surface_percentile=100)
    np.testing.assert_array_equal(full["hausdorff_percentile_distances"], base["hausdorff_distances"])
    host = ev.evaluate_model(net, loader, dev, surface_metrics=True, surface_percentile=90, surface_tolerance=3,
                             surface_backend="host")
    np.testing.assert_array_equal(host["hausdorff_percentile_distances"], got["hausdorff_percentile_distances"])
    np.testing.assert_allclose(host["assd_distances"], got["assd_distances"], rtol=1e-12)
    for kw in (dict(surface_percentile=0), dict(surface_tolerance=-1), dict(surface_backend="gpu")):
        with pytest.raises(ValueError):
            ev.evaluate_model(net, loader, dev, surface_metrics=True, **kw)


def test_eval_cli_surface_columns(hip, tmp_path):
    import evaluate as eval_cli
    from PIL import Image
    from physics_informed_image_segmentation_amd import UNet
    d = tmp_path / "testing"
    d.mkdir()
    imgs, anns = [], []
    for i in range(3):
        a = np.full((64, 64), 40, np.uint8)
        x0, y0 = 8 + 6 * i, 10 + 4 * i
        a[y0:y0 + 20, x0:x0 + 24] = 200
        Image.fromarray(a, mode="L").save(d / f"{i}.png")
        imgs.append({"id": i, "file_name": f"{i}.png", "height": 64, "width": 64})
        anns.append({"id": 100 + i, "image_id": i,
                     "segmentation": [[x0, y0, x0 + 23, y0, x0 + 23, y0 + 19, x0, y0 + 19]]})
    js = tmp_path / "test.json"
    js.write_text(json.dumps({"images": imgs, "annotations": anns}))
    paths = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        path = tmp_path / f"m{seed}.pth"
        torch.save(UNet(1, 1, 64).state_dict(), path)
        paths.append(path)
    res = eval_cli.main(["--baseline", str(paths[0]), "--pde", str(paths[1]), "--test-dir", str(d), "--test-json",
                         str(js), "--batch-size", "2", "--device-cache", "--output-dir", str(tmp_path / "surf"),
                         "--surface-metrics", "--surface-percentile", "90"])
    old_keys = ["dice_scores", "iou_scores", "boundary_f1_scores", "hausdorff_distances"]
    old_header = ["image_id", "baseline_dice", "pde_dice", "baseline_iou", "pde_iou", "baseline_boundary_f1",
                  "pde_boundary_f1", "baseline_hausdorff", "pde_hausdorff"]
    new_keys = old_keys + list(ev.SURFACE_METRIC_KEYS)
    assert list(res["baseline_metrics"]) == new_keys and list(res["pde_metrics"]) == new_keys
    assert open(res["results_csv"]).readline().strip().split(",") == old_header + [
        "baseline_hausdorff_percentile", "pde_hausdorff_percentile", "baseline_assd", "pde_assd",
        "baseline_surface_dice", "pde_surface_dice"]
    assert list(json.load(open(res["comparison_json"]))) == new_keys
    assert all(len(res["baseline_metrics"][k]) == 3 for k in new_keys)
