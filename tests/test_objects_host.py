"""Object-level metrics (evaluate.py: object_counts, label_components, compute_object_f1_batch,
compute_aji_batch) on a GPU-less host: the scipy / numpy path against hand-computed answers, the
argument checks of the Python surface and of pis_object_metrics before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd import evaluate as ev


def _counts(p, t, **kw):
    c = ev.object_counts(torch.from_numpy(p)[None], torch.from_numpy(t)[None], **kw)
    assert c.dtype == torch.int64 and c.shape == (1, 8) and c.device.type == "cpu"
    return c[0].tolist()


def case_a():
    t = np.zeros((6, 8), np.float32)
    p = np.zeros((6, 8), np.float32)
    t[1:3, 1:3] = 1
    t[4, 4:8] = 1
    p[1:3, 1] = 1
    p[4, 5:8] = 1
    p[0, 7] = 1
    return p, t


def case_b():
    t = np.zeros((6, 8), np.float32)
    p = np.zeros((6, 8), np.float32)
    t[2, 0:3] = 1
    t[2, 4:8] = 1
    p[2, 1:7] = 1
    return p, t


def case_c():
    m = np.zeros((64, 64), np.float32)
    for y, x in ((31, 31), (32, 32), (31, 40), (32, 39)):
        m[y, x] = 1
    return m, m.copy()


def checkerboard(H=33, W=47):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2).astype(np.float32)


def test_case_a_thresholds_are_strict():
    """Square 2x2 against its left column: IoU = 2 / 4 = 0.5 is not a match. Bar of 4 against 3 of
    it: IoU = 0.75 counts at 0.5 only. The speck (0, 7) is a false positive and enters the AJI
    union; with min_area = 2 it is removed and leaves it."""
    p, t = case_a()
    assert _counts(p, t) == [3, 2, 1, 0, 5, 9, 6, 0]
    assert _counts(p, t, min_area=2) == [2, 2, 1, 0, 5, 8, 5, 1]
    # the speck is (0, 7): the first predicted object in row-major order
    lab, n = ev.label_components(torch.from_numpy(p)[None], threshold=0.5)
    assert n.tolist() == [3] and lab[0, 0, 7] == 1 and lab[0, 1, 1] == 2 and lab[0, 4, 5] == 3


def test_case_b_one_prediction_bridges_two_cells():
    """I / U = 2 / 7 and 3 / 7: the prediction is the best match of both cells, so its union is
    added twice (7 + 7) and nothing is left unused."""
    assert _counts(*case_b()) == [1, 2, 0, 0, 5, 14, 6, 0]


def test_case_c_diagonals_at_a_tile_corner():
    p, t = case_c()
    assert _counts(p, t, connectivity=8) == [2, 2, 2, 2, 4, 4, 4, 0]
    assert _counts(p, t, connectivity=4) == [4, 4, 4, 4, 4, 4, 4, 0]


def test_case_d_checkerboard():
    cb = checkerboard()
    assert int(cb.sum()) == 775
    assert _counts(cb, cb, connectivity=4) == [775] * 7 + [0]
    assert _counts(cb, cb, connectivity=8) == [1, 1, 1, 1, 775, 775, 775, 0]
    assert _counts(cb, 1 - cb, connectivity=8) == [1, 1, 0, 0, 0, 1551, 775, 0]


def test_numbering_follows_the_first_pixel():
    """A U whose right arm starts one row above the left arm is one object under both
    connectivities; a dot to its left starts between the two arms' first pixels. The numbering goes
    by the first pixel of the whole object: the U (first pixel (1, 6)) is 1, the dot (2, 0) is 2."""
    m = np.zeros((8, 9), np.float32)
    m[2:6, 2] = 1   # left arm from row 2
    m[1:6, 6] = 1   # right arm from row 1
    m[5, 2:7] = 1   # bottom
    m[2, 0] = 1     # dot
    for conn in (4, 8):
        lab, n = ev.label_components(torch.from_numpy(m)[None], connectivity=conn)
        assert lab.dtype == torch.int32 and lab.shape == (1, 8, 9) and n.dtype == torch.int64
        assert n.tolist() == [2]
        lab = lab[0].numpy()
        assert lab[1, 6] == 1 and lab[2, 2] == 1 and lab[5, 4] == 1 and lab[2, 0] == 2
        assert (lab > 0).sum() == m.sum()


def test_area_equal_to_min_area_is_kept():
    m = np.zeros((5, 9), np.float32)
    m[1, 1:4] = 1      # 3 pixels
    m[3, 5:7] = 1      # 2 pixels
    lab, n = ev.label_components(torch.from_numpy(m)[None], min_area=3)
    assert n.tolist() == [1] and lab[0, 1, 2] == 1 and lab[0, 3, 5] == 0
    lab, n = ev.label_components(torch.from_numpy(m)[None], min_area=2)
    assert n.tolist() == [2] and lab[0, 3, 5] == 2
    assert ev.label_components(torch.from_numpy(m)[None], min_area=4)[1].tolist() == [0]
    # targets are never filtered
    assert _counts(m, m, min_area=3) == [1, 2, 1, 1, 3, 5, 3, 1]


def test_empty_and_full_images():
    z, o = np.zeros((7, 5), np.float32), np.ones((7, 5), np.float32)
    assert _counts(z, z) == [0] * 8
    assert _counts(o, o) == [1, 1, 1, 1, 35, 35, 35, 0]
    assert _counts(o, z) == [1, 0, 0, 0, 0, 35, 35, 0]
    assert _counts(z, o) == [0, 1, 0, 0, 0, 35, 0, 0]
    assert _counts(o[:1, :1], o[:1, :1], connectivity=4) == [1, 1, 1, 1, 1, 1, 1, 0]


def test_nan_is_background():
    p = np.ones((4, 6), np.float32)
    p[:, 3] = np.nan  # a NaN column cuts the prediction in two
    t = np.ones((4, 6), np.float32)
    assert _counts(p, t) == [2, 1, 0, 0, 12, 32, 20, 0]
    lab, n = ev.label_components(torch.from_numpy(p)[None], threshold=0.5)
    assert n.tolist() == [2] and (lab[0, :, 3] == 0).all()


def test_scores():
    p, t = case_a()
    tp, tt = torch.from_numpy(np.stack([p, np.zeros_like(p)])), torch.from_numpy(np.stack([t, np.zeros_like(t)]))
    f50 = ev.compute_object_f1_batch(tp, tt)
    f75 = ev.compute_object_f1_batch(tp, tt, iou=0.75)
    aji = ev.compute_aji_batch(tp, tt)
    for s in (f50, f75, aji):
        assert s.dtype == torch.float64 and s.shape == (2,)
        assert np.isnan(s[1].item())  # no predicted and no true object
    assert f50[0].item() == 2 * 1 / 5 and f75[0].item() == 0.0 and aji[0].item() == 5 / 9
    # one side empty is a plain zero, not NaN
    assert ev.compute_object_f1_batch(tp[:1], tt[1:]).item() == 0.0
    assert ev.compute_aji_batch(tp[:1], tt[1:]).item() == 0.0
    assert ev.compute_statistics(np.append(aji.numpy(), 1.0))["count"] == 2  # NaN is skipped


def test_batch_shapes():
    p, t = case_a()
    c3 = ev.object_counts(torch.from_numpy(np.stack([p, t, p])), torch.from_numpy(np.stack([t, t, p])))
    assert c3.shape == (3, 8) and c3[0].tolist() == [3, 2, 1, 0, 5, 9, 6, 0]
    assert c3[1].tolist() == [2, 2, 2, 2, 8, 8, 8, 0] and c3[2].tolist() == [3, 3, 3, 3, 6, 6, 6, 0]
    c4 = ev.object_counts(torch.from_numpy(p)[None, None], torch.from_numpy(t)[None, None])
    assert c4.tolist() == [c3[0].tolist()]


def test_bad_arguments_raise():
    p, t = (torch.from_numpy(a)[None] for a in case_a())
    for kw in (dict(connectivity=6), dict(connectivity=0), dict(min_area=-1), dict(min_area=1.5),
               dict(backend="gpu"), dict(backend="device")):
        with pytest.raises(ValueError):
            ev.object_counts(p, t, **kw)
        with pytest.raises(ValueError):
            ev.compute_aji_batch(p, t, **kw)
        with pytest.raises(ValueError):
            ev.label_components(p, **kw)
    with pytest.raises(ValueError):
        ev.compute_object_f1_batch(p, t, iou=0.6)
    with pytest.raises(ValueError):
        ev.object_counts(p, t[:, :4])


def test_facade_exports():
    import physics_informed_image_segmentation_amd as pkg
    import src
    from physics_informed_image_segmentation_amd import evaluate_comparison as ec
    for name in ("object_counts", "label_components", "compute_object_f1_batch", "compute_aji_batch"):
        assert getattr(pkg, name) is getattr(ev, name) is getattr(src, name)
        assert name in pkg.__all__
    assert ec.METRIC_KEYS == ("dice_scores", "iou_scores", "boundary_f1_scores", "hausdorff_distances")
    assert ec.OBJECT_METRIC_KEYS == ("object_f1_scores", "aji_scores", "object_count_errors")


def test_cli_flags():
    import evaluate as eval_cli
    a = eval_cli.parse_args(["--baseline", "b.pth", "--pde", "p.pth"])
    assert (a.object_metrics, a.connectivity, a.min_object_area) == (False, 8, 0)
    a = eval_cli.parse_args(["--baseline", "b.pth", "--pde", "p.pth", "--object-metrics", "--connectivity", "4",
                             "--min-object-area", "12"])
    assert (a.object_metrics, a.connectivity, a.min_object_area) == (True, 4, 12)
    with pytest.raises(SystemExit):
        eval_cli.parse_args(["--baseline", "b.pth", "--pde", "p.pth", "--connectivity", "6"])


def test_comparison_files_carry_the_object_metrics_only_when_switched_on(tmp_path, monkeypatch):
    """evaluate_and_compare / run_repeated_evaluations with the model and the test-set evaluation
    stubbed out: the switch reaches evaluate_on_test_set, and the per-image columns, the summary
    rows and the aggregated rows grow by the three object metrics only when it is on."""
    from physics_informed_image_segmentation_amd import evaluate_comparison as ec
    seen = []

    def fake_eval(model, test_dir, test_json, device, batch_size=8, threshold=0.5, model_name="Model",
                  device_cache=False, object_metrics=False, connectivity=8, min_object_area=0):
        seen.append((object_metrics, connectivity, min_object_area))
        g = np.random.default_rng(len(seen))
        keys = ec.METRIC_KEYS + (ec.OBJECT_METRIC_KEYS if object_metrics else ())
        return {k: g.random(5) for k in keys}

    monkeypatch.setattr(ec, "load_model", lambda path, device: None)
    monkeypatch.setattr(ec, "evaluate_on_test_set", fake_eval)
    base_cols = ["image_id", "baseline_dice", "pde_dice", "baseline_iou", "pde_iou", "baseline_boundary_f1",
                 "pde_boundary_f1", "baseline_hausdorff", "pde_hausdorff"]
    obj_cols = ["baseline_object_f1", "pde_object_f1", "baseline_aji", "pde_aji", "baseline_object_count_error",
                "pde_object_count_error"]
    args = ("b.pth", "p.pth", "dir", "json", torch.device("cpu"))
    off = ec.evaluate_and_compare(*args, output_dir=tmp_path / "off")
    on = ec.evaluate_and_compare(*args, output_dir=tmp_path / "on", object_metrics=True, connectivity=4,
                                 min_object_area=7)
    assert seen == [(False, 8, 0)] * 2 + [(True, 4, 7)] * 2
    assert open(off["results_csv"]).readline().strip().split(",") == base_cols
    assert open(on["results_csv"]).readline().strip().split(",") == base_cols + obj_cols
    rows = lambda path: [line.split(",")[0] for line in open(path).read().splitlines()[1:]]  # noqa: E731
    assert rows(off["summary_csv"]) == list(ec.METRIC_KEYS)
    assert rows(on["summary_csv"]) == list(ec.METRIC_KEYS + ec.OBJECT_METRIC_KEYS)
    assert set(off["comparison_results"]) == set(ec.METRIC_KEYS)
    assert set(on["comparison_results"]) == set(ec.METRIC_KEYS + ec.OBJECT_METRIC_KEYS)
    rargs = (["b1", "b2"], ["p1", "p2"], "dir", "json", torch.device("cpu"))
    off = ec.run_repeated_evaluations(*rargs, output_dir=tmp_path / "roff")
    on = ec.run_repeated_evaluations(*rargs, output_dir=tmp_path / "ron", object_metrics=True)
    assert seen[-4:] == [(True, 8, 0)] * 4
    assert open(on["aggregated_csv"]).readline().strip() == "metric,model,mean,std,count"
    assert rows(off["aggregated_csv"]) == [k for k in ec.METRIC_KEYS for _ in range(2)]
    assert rows(on["aggregated_csv"]) == [k for k in ec.METRIC_KEYS + ec.OBJECT_METRIC_KEYS for _ in range(2)]
    assert len(on["baseline_metrics"]["aji_scores"]) == 10 and set(off["baseline_metrics"]) == set(ec.METRIC_KEYS)


# ---------------------------------------------------------------------------- C ABI, before any launch

def test_symbols_and_workspace_query():
    lib = _hip.lib()
    for name in ("pis_objects_ws", "pis_object_metrics"):
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    n = lib.pis_objects_ws(8, 512, 512)
    # label, area and auxiliary slot per pixel of the 16 images; a table of 2 * H * W / 2 slots of
    # 12 bytes per sample (the worst case: a 4-connectivity checkerboard, one pair per run)
    assert n >= 3 * 4 * 16 * 512 * 512 + 8 * 512 * 512 * 12
    assert lib.pis_objects_ws(1, 1, 1) > 0 and lib.pis_objects_ws(1, 4096, 4096) > 0
    assert lib.pis_objects_ws(1, 4097, 16) == 0 and lib.pis_objects_ws(1, 16, 4097) == 0
    assert lib.pis_objects_ws(0, 16, 16) == 0 and lib.pis_objects_ws(1, 0, 16) == 0


def _call(p=1, t=1, B=1, H=16, W=16, conn=8, min_area=0, counts=1, ws=1, ws_bytes=None):
    """pis_object_metrics with host buffers standing in for device memory: every case here must be
    refused before any launch, so nothing dereferences them."""
    lib = _hip.lib()
    n = max(B, 1) * 16 * 16
    fp = (ctypes.c_float * n)()
    ft = (ctypes.c_float * n)()
    c = (ctypes.c_int64 * (8 * max(B, 1)))()
    need = lib.pis_objects_ws(1, 16, 16)
    w = (ctypes.c_uint8 * need)()
    addr = lambda on, buf: ctypes.addressof(buf) if on else 0  # noqa: E731
    rc = lib.pis_object_metrics(addr(p, fp), addr(t, ft), B, H, W, 0.5, conn, min_area, addr(counts, c), 0, 0,
                                addr(ws, w), need if ws_bytes is None else ws_bytes, 0)
    return rc, lib.pis_last_error()


@pytest.mark.parametrize("kw", [dict(p=0), dict(t=0), dict(counts=0), dict(ws=0), dict(B=0), dict(W=4097),
                                dict(H=4097), dict(H=0), dict(conn=6), dict(conn=0), dict(min_area=-1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_argument_errors_are_reported_before_any_launch(kw):
    rc, msg = _call(**kw)
    assert rc == -1
    assert b"pis_object_metrics" in msg


def test_short_workspace_is_a_workspace_error():
    rc, msg = _call(ws_bytes=16)
    assert rc == -3
    assert b"pis_object_metrics" in msg
