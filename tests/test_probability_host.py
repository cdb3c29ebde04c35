"""Probability-level metrics (evaluate.py: probability_table, threshold_sweep_counts, AUROC, average
precision, ECE, Brier, best threshold, ProbabilityTable) on a GPU-less host: the numpy path against
hand-computed answers, the argument checks of the Python surface and of pis_probability_table
before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd import evaluate as ev

NEXT = np.nextafter(np.float32(0.5), np.float32(1.0))


def hand_case():
    """2 x 4 image. Pixel: p -> q, bin | target
       0: 0      -> 0,     0    | 0        4: 0.75 -> 49152, 768  | 1
       1: 0.25   -> 16384, 256  | 0        5: 1    -> 65536, 1024 | 1
       2: 0.5    -> 32768, 512  | 1        6: NaN  -> 0,     0    | 1
       3: 0.5+   -> 32769, 513  | 0        7: 0.1  -> 6554,  103  | 0
    (0.1f * 65536 = 6553.6001: ceil 6554, (6554 + 63) >> 6 = 103)."""
    p = np.array([[0, 0.25, 0.5, NEXT], [0.75, 1, np.nan, 0.1]], np.float32)
    t = np.array([[0, 0, 1, 0], [1, 1, 1, 0]], np.float32)
    return torch.from_numpy(p)[None], torch.from_numpy(t)[None]


def test_hand_case_table():
    p, t = hand_case()
    table, extra = ev.probability_table(p, t)
    assert table.dtype == torch.int64 and table.shape == (1, 2, 1025, 2) and table.device.type == "cpu"
    assert extra.dtype == torch.int64 and extra.shape == (1, 4)
    want = np.zeros((2, 1025, 2), np.int64)
    for cls, b, q in ((0, 0, 0), (0, 256, 16384), (1, 512, 32768), (0, 513, 32769), (1, 768, 49152),
                      (1, 1024, 65536), (1, 0, 0), (0, 103, 6554)):
        want[cls, b] += (1, q)
    np.testing.assert_array_equal(table[0].numpy(), want)
    assert extra[0].tolist() == [16384 ** 2 + 32769 ** 2 + 6554 ** 2, 32768 ** 2 + 49152 ** 2 + 65536 ** 2, 1, 0]
    # (B, 1, H, W) is accepted like (B, H, W)
    t4, e4 = ev.probability_table(p[:, None], t[:, None])
    assert torch.equal(t4, table) and torch.equal(e4, extra)


def test_hand_case_sweep_and_best_threshold():
    p, t = hand_case()
    table, _ = ev.probability_table(p, t)
    sweep = ev.threshold_sweep_counts(table)
    assert sweep.dtype == torch.int64 and sweep.shape == (1, 1024, 3)
    # rows (I_hat, P_hat, T): the bins above j are counted
    assert sweep[0, 0].tolist() == [3, 6, 4]       # p > 0: all but the zero and the NaN
    assert sweep[0, 255].tolist() == [3, 5, 4]     # 0.1 has left
    assert sweep[0, 256].tolist() == [3, 4, 4]     # p > 0.25 is strict: 0.25 has left
    assert sweep[0, 512].tolist() == [2, 3, 4]     # p > 0.5: 0.5 itself has left, its upper neighbour stays
    assert sweep[0, 1023].tolist() == [1, 1, 4]    # only p = 1 is above 1023 / 1024
    # Dice per row: 6 / 10, 6 / 9 (j >= 103), 6 / 8 from j = 256 to 511, then 4 / 7 ...: the first best is 256
    thr, dice = ev.best_threshold_batch(table)
    assert thr.dtype == torch.float64 and thr.tolist() == [0.25]
    assert dice.tolist() == [(2.0 * 3 + 1e-6) / (4 + 4 + 1e-6)]
    thr2, dice2 = ev.best_threshold_batch(p, t)
    assert torch.equal(thr, thr2) and torch.equal(dice, dice2)


def test_hand_case_scores():
    p, t = hand_case()
    table, extra = ev.probability_table(p, t)
    # AUROC: positives at bins 512, 768, 1024, 0 against negatives at 0, 103, 256, 513:
    # 3 + 4 + 4 pairs won and one tie (the NaN against the zero): 11.5 / 16
    assert ev.compute_auroc_batch(table).tolist() == [23 / 32]
    # AP, bins from the top: (1/4) (1/1) + (1/4) (2/2) + (1/4) (3/4) [bin 513 is a negative] + (1/4) (4/8)
    assert ev.compute_average_precision_batch(table).tolist() == [0.25 + 0.25 + 0.1875 + 0.125]
    # ECE with 2 bins: bins 0..512 hold q = 0, 16384, 32768, 0, 6554 with 2 positives, bins 513..1024 hold
    # 32769, 49152, 65536 with 2 positives
    ece2 = abs(55706 - 2 * 65536) + abs(147457 - 2 * 65536)
    assert ece2 == 91751
    assert ev.compute_ece_batch(table, n_bins=2).tolist() == [ece2 / (65536 * 8)]
    # 16 bins of 64 fine bins: {0, NaN} -> 0 (1 positive), 103 -> 1, 256 -> 3, 512 -> 7 (positive),
    # 513 -> 8, 768 -> 11 (positive), 1024 -> 15 (positive)
    ece16 = 65536 + 6554 + 16384 + (65536 - 32768) + 32769 + (65536 - 49152) + 0
    assert ece16 == 170395
    assert ev.compute_ece_batch(table).tolist() == [ece16 / (65536 * 8)]
    assert ev.compute_ece_batch(p, t, n_bins=16).tolist() == [ece16 / (65536 * 8)]
    # Brier: sum of (q - 65536 cls)^2 over the eight pixels
    num = 0 + 16384 ** 2 + 32768 ** 2 + 32769 ** 2 + 16384 ** 2 + 0 + 65536 ** 2 + 6554 ** 2
    assert num == 7022342309
    assert ev.compute_brier_batch((table, extra)).tolist() == [num / (2 ** 32 * 8)]
    assert ev.compute_brier_batch(p, t).tolist() == [num / (2 ** 32 * 8)]
    for s in (ev.compute_auroc_batch(p, t), ev.compute_average_precision_batch(p, t), ev.compute_brier_batch(p, t)):
        assert s.dtype == torch.float64 and s.shape == (1,)


def test_quantisation_edges():
    """p > j / 1024 holds exactly when bin > j: at the grid values, their float neighbours, zeros,
    denormals, values outside [0, 1] and the non-finite ones."""
    j = np.arange(1025, dtype=np.float32) / np.float32(1024)
    vals = np.concatenate([j, np.nextafter(j, np.float32(-1)), np.nextafter(j, np.float32(2)),
                           np.array([0.0, -0.0, 1e-45, 1e-40, -1e-45, -0.3, 1.5, 3e38, np.inf, -np.inf, np.nan],
                                    np.float32)]).astype(np.float32)
    p = torch.from_numpy(vals)[None, None]
    table, extra = ev.probability_table(p, torch.zeros_like(p))
    sweep = ev.threshold_sweep_counts(table)[0, :, 1].numpy()
    with np.errstate(invalid="ignore"):
        want = np.array([(vals > np.float32(k) / np.float32(1024)).sum() for k in range(1024)])
    np.testing.assert_array_equal(sweep, want)
    assert extra[0, 2].item() == 1 and table[0, 1].sum().item() == 0
    # bin 0 holds q = 0 only; above 1 and +Inf give q = 65536
    assert table[0, 0, 0, 1].item() == 0
    n_top = int((vals >= 1).sum()) + 1  # and the lower neighbour of 1 (q = 65535 is in bin 1024 too)
    assert table[0, 0, 1024, 0].item() >= n_top


def test_degenerate_samples():
    g = torch.Generator().manual_seed(3)
    p = torch.rand(3, 5, 7, generator=g)
    t = torch.stack([torch.ones(5, 7), torch.zeros(5, 7), (torch.rand(5, 7, generator=g) > 0.5).float()])
    auroc = ev.compute_auroc_batch(p, t)
    ap = ev.compute_average_precision_batch(p, t)
    assert np.isnan(auroc[0].item()) and np.isnan(auroc[1].item()) and 0 <= auroc[2].item() <= 1
    assert abs(ap[0].item() - 1.0) < 1e-12 and np.isnan(ap[1].item()) and 0 < ap[2].item() <= 1
    assert np.isfinite(ev.compute_ece_batch(p, t).numpy()).all()
    assert np.isfinite(ev.compute_brier_batch(p, t).numpy()).all()
    assert ev.compute_statistics(auroc.numpy())["count"] == 1  # NaN is skipped downstream


def test_row_512_is_the_plain_threshold():
    rng = np.random.default_rng(5)
    p = rng.random((3, 33, 47)).astype(np.float32)
    p[0, :4] = 0.5
    p[1, 5] = np.nan
    t = (rng.random((3, 33, 47)) > 0.6).astype(np.float32)
    t[2, 3] = 0.5   # not above 0.5: class 0
    table, _ = ev.probability_table(torch.from_numpy(p), torch.from_numpy(t))
    row = ev.threshold_sweep_counts(table)[:, 512].numpy()
    with np.errstate(invalid="ignore"):
        pb, tb = p > 0.5, t > 0.5
    want = np.stack([(pb & tb).sum((1, 2)), pb.sum((1, 2)), tb.sum((1, 2))], axis=1)
    np.testing.assert_array_equal(row, want)
    # and scores against their direct definitions on q / 65536
    q = np.where(np.isnan(p), 0, np.ceil(p.astype(np.float64) * 65536)).clip(0, 65536) / 65536
    brier = ((q - tb) ** 2).mean((1, 2))
    np.testing.assert_allclose(ev.compute_brier_batch(torch.from_numpy(p), torch.from_numpy(t)).numpy(), brier,
                               rtol=1e-12)


def test_pooling_two_batches_equals_one():
    rng = np.random.default_rng(7)
    p = torch.from_numpy(rng.random((5, 16, 20)).astype(np.float32))
    t = torch.from_numpy((rng.random((5, 16, 20)) > 0.5).astype(np.float32))
    one = ev.ProbabilityTable().update(*ev.probability_table(p, t))
    two = ev.ProbabilityTable()
    assert two.total_count == 0
    two.update(*ev.probability_table(p[3:], t[3:]))
    two.update(*ev.probability_table(p[:3], t[:3]))
    assert torch.equal(one.table, two.table) and torch.equal(one.extra, two.extra)
    assert one.table.shape == (2, 1025, 2) and one.total_count == 5 * 16 * 20
    # the pooled table is the table of all pixels as one sample
    flat = ev.probability_table(p.reshape(1, 1, -1), t.reshape(1, 1, -1))
    assert torch.equal(one.table, flat[0][0]) and torch.equal(one.extra, flat[1][0])
    sw = one.sweep()
    assert set(sw) == {"threshold", "tp", "fp", "fn", "precision", "recall", "dice", "iou"}
    assert all(v.shape == (1024,) for v in sw.values())
    assert sw["threshold"][512].item() == 0.5
    pb, tb = p > 0.5, t > 0.5
    assert sw["tp"][512].item() == (pb & tb).sum().item() and sw["fp"][512].item() == (pb & ~tb).sum().item()
    assert sw["fn"][512].item() == (~pb & tb).sum().item()
    assert sw["precision"][512].item() == (pb & tb).sum().item() / pb.sum().item()
    thr, dice = one.best_threshold()
    assert dice == sw["dice"].max().item() and thr == sw["threshold"][int(sw["dice"].argmax())].item()
    rel = one.reliability(4)
    assert rel["count"].tolist() == [int(((p > lo) & (p <= lo + 0.25)).sum()) for lo in (0, 0.25, 0.5, 0.75)]
    assert rel["count"].sum().item() == one.total_count
    np.testing.assert_allclose(rel["mean_confidence"].numpy(), [0.125, 0.375, 0.625, 0.875], atol=0.02)
    np.testing.assert_allclose(rel["positive_fraction"].numpy(), 0.5, atol=0.1)
    assert one.ece(4) == ev.compute_ece_batch(flat[0], n_bins=4).item()
    assert one.brier() == ev.compute_brier_batch(flat).item()
    assert one.auroc() == ev.compute_auroc_batch(flat[0]).item()
    assert one.average_precision() == ev.compute_average_precision_batch(flat[0]).item()
    with pytest.raises(ValueError):
        ev.ProbabilityTable().sweep()


def test_bad_arguments_raise():
    p, t = hand_case()
    table, extra = ev.probability_table(p, t)
    for n in (0, 3, 12, 2048, -4, 1.5, True):
        with pytest.raises(ValueError):
            ev.compute_ece_batch(table, n_bins=n)
        with pytest.raises(ValueError):
            ev.ProbabilityTable().update(table, extra).reliability(n)
        with pytest.raises(ValueError):
            ev.evaluate_model(None, [], torch.device("cpu"), probability_metrics=True, calibration_bins=n)
    for n in (1, 2, 16, 1024):
        assert ev.compute_ece_batch(table, n_bins=n).shape == (1,)
    for kw in (dict(backend="gpu"), dict(backend="device")):
        with pytest.raises(ValueError):
            ev.probability_table(p, t, **kw)
        with pytest.raises(ValueError):
            ev.compute_auroc_batch(p, t, **kw)
    with pytest.raises(ValueError):
        ev.probability_table(p, t[:, :1])
    with pytest.raises(ValueError):
        ev.compute_brier_batch(table)             # needs the sums of squares
    with pytest.raises(ValueError):
        ev.threshold_sweep_counts(table[:, :, :1000])
    with pytest.raises(ValueError):
        ev.compute_auroc_batch(table.to(torch.int32))


def test_sklearn_agrees_on_the_bin_index():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(11)
    p = rng.random(5000).astype(np.float32)
    t = (rng.random(5000) < 0.3 + 0.4 * p).astype(np.float32)
    tp, tt = torch.from_numpy(p).reshape(1, 50, 100), torch.from_numpy(t).reshape(1, 50, 100)
    b = np.ceil(p.astype(np.float64) * 1024)
    np.testing.assert_allclose(ev.compute_auroc_batch(tp, tt).item(), sk.roc_auc_score(t, b), rtol=1e-12)
    np.testing.assert_allclose(ev.compute_average_precision_batch(tp, tt).item(),
                               sk.average_precision_score(t, b), rtol=1e-12)


# ---------------------------------------------------------------------------- wiring

def test_facade_exports():
    import physics_informed_image_segmentation_amd as pkg
    import src
    from physics_informed_image_segmentation_amd import evaluate_comparison as ec
    for name in ("probability_table", "threshold_sweep_counts", "compute_auroc_batch",
                 "compute_average_precision_batch", "compute_ece_batch", "compute_brier_batch",
                 "best_threshold_batch", "ProbabilityTable"):
        assert getattr(pkg, name) is getattr(ev, name) is getattr(src, name)
        assert name in pkg.__all__ and name in ev.__all__
    # the keyword arguments the comparison functions pass on exist, off by default
    import inspect
    for fn in (ev.evaluate_model, ev.evaluate_on_test_set):
        par = inspect.signature(fn).parameters
        assert (par["probability_metrics"].default, par["calibration_bins"].default,
                par["probability_table"].default) == (False, 16, None)
    for fn in (ec.evaluate_and_compare, ec.run_repeated_evaluations):
        par = inspect.signature(fn).parameters
        assert (par["probability_metrics"].default, par["calibration_bins"].default) == (False, 16)
    assert ec.PROBABILITY_METRIC_KEYS == ev.PROBABILITY_METRIC_KEYS == (
        "auroc_scores", "average_precision_scores", "ece_scores", "brier_scores", "best_threshold_dice_scores",
        "best_thresholds")


def test_cli_flags():
    import evaluate as eval_cli
    a = eval_cli.parse_args(["--baseline", "b.pth", "--pde", "p.pth"])
    assert (a.probability_metrics, a.calibration_bins) == (False, 16)
    a = eval_cli.parse_args(["--baseline", "b.pth", "--pde", "p.pth", "--probability-metrics",
                             "--calibration-bins", "32"])
    assert (a.probability_metrics, a.calibration_bins) == (True, 32)
    for bad in ("12", "0", "2048"):
        with pytest.raises(SystemExit):
            eval_cli.parse_args(["--baseline", "b.pth", "--pde", "p.pth", "--calibration-bins", bad])


def test_comparison_files_carry_the_probability_metrics_only_when_switched_on(tmp_path, monkeypatch):
    """evaluate_and_compare / run_repeated_evaluations with the model and the test-set evaluation
    stubbed out: columns, rows and files grow only with the switch on, and the stub without the new
    keyword arguments still serves the switched-off call."""
    import json

    from physics_informed_image_segmentation_amd import evaluate_comparison as ec
    seen = []

    def old_eval(model, test_dir, test_json, device, batch_size=8, threshold=0.5, model_name="Model",
                 device_cache=False, object_metrics=False, connectivity=8, min_object_area=0):
        g = np.random.default_rng(1)
        return {k: g.random(5) for k in ec.METRIC_KEYS}

    def new_eval(model, test_dir, test_json, device, batch_size=8, threshold=0.5, model_name="Model",
                 device_cache=False, object_metrics=False, connectivity=8, min_object_area=0,
                 probability_metrics=False, calibration_bins=16, probability_table=None):
        seen.append((probability_metrics, calibration_bins, probability_table is not None))
        g = np.random.default_rng(len(seen))
        if probability_table is not None:
            p = torch.from_numpy(g.random((2, 8, 8)).astype(np.float32))
            probability_table.update(*ev.probability_table(p, (p > 0.4).float()))
        keys = ec.METRIC_KEYS + (ec.PROBABILITY_METRIC_KEYS if probability_metrics else ())
        return {k: g.random(5) for k in keys}

    monkeypatch.setattr(ec, "load_model", lambda path, device: None)
    args = ("b.pth", "p.pth", "dir", "json", torch.device("cpu"))
    base_cols = ["image_id", "baseline_dice", "pde_dice", "baseline_iou", "pde_iou", "baseline_boundary_f1",
                 "pde_boundary_f1", "baseline_hausdorff", "pde_hausdorff"]
    prob_cols = [f"{m}_{c}" for c in ("auroc", "average_precision", "ece", "brier", "best_threshold_dice",
                                      "best_threshold") for m in ("baseline", "pde")]
    monkeypatch.setattr(ec, "evaluate_on_test_set", old_eval)
    off = ec.evaluate_and_compare(*args, output_dir=tmp_path / "off")
    assert open(off["results_csv"]).readline().strip().split(",") == base_cols
    assert set(json.load(open(off["comparison_json"]))) == set(ec.METRIC_KEYS)
    assert sorted(f.name.split("_2")[0] for f in (tmp_path / "off").iterdir()) == [
        "evaluation_results", "evaluation_summary", "statistical_comparison"]
    assert set(off) == {"baseline_metrics", "pde_metrics", "comparison_results", "results_csv", "summary_csv",
                        "comparison_json"}
    monkeypatch.setattr(ec, "evaluate_on_test_set", new_eval)
    on = ec.evaluate_and_compare(*args, output_dir=tmp_path / "on", probability_metrics=True, calibration_bins=8)
    assert seen == [(True, 8, True)] * 2
    assert open(on["results_csv"]).readline().strip().split(",") == base_cols + prob_cols
    rows = lambda path: [line.split(",")[0] for line in open(path).read().splitlines()[1:]]  # noqa: E731
    assert rows(on["summary_csv"]) == list(ec.METRIC_KEYS + ec.PROBABILITY_METRIC_KEYS)
    js = json.load(open(on["comparison_json"]))
    assert set(js) == set(ec.METRIC_KEYS + ec.PROBABILITY_METRIC_KEYS) | {"pooled_best_threshold"}
    assert set(js["pooled_best_threshold"]) == {"baseline", "pde"}
    assert 0 <= js["pooled_best_threshold"]["pde"]["threshold"] < 1
    assert set(on["comparison_results"]) == set(ec.METRIC_KEYS + ec.PROBABILITY_METRIC_KEYS)
    for tag in ("baseline", "pde"):
        sweep = open(on[f"threshold_sweep_{tag}_csv"]).read().splitlines()
        assert sweep[0] == "threshold,tp,fp,fn,precision,recall,dice,iou" and len(sweep) == 1025
        assert sweep[513].startswith("0.5,")
        rel = open(on[f"reliability_{tag}_csv"]).read().splitlines()
        assert rel[0] == "bin,count,mean_confidence,positive_fraction" and len(rel) == 9
    rargs = (["b1", "b2"], ["p1", "p2"], "dir", "json", torch.device("cpu"))
    ron = ec.run_repeated_evaluations(*rargs, output_dir=tmp_path / "ron", probability_metrics=True)
    assert seen[-4:] == [(True, 16, False)] * 4
    assert rows(ron["aggregated_csv"]) == [k for k in ec.METRIC_KEYS + ec.PROBABILITY_METRIC_KEYS for _ in range(2)]
    monkeypatch.setattr(ec, "evaluate_on_test_set", old_eval)
    roff = ec.run_repeated_evaluations(*rargs, output_dir=tmp_path / "roff")
    assert rows(roff["aggregated_csv"]) == [k for k in ec.METRIC_KEYS for _ in range(2)]


# ---------------------------------------------------------------------------- C ABI, before any launch

def test_symbols_and_workspace_query():
    lib = _hip.lib()
    for name in ("pis_probability_ws", "pis_probability_table"):
        assert name in _hip.exported_symbols() and hasattr(lib, name)
    assert lib.pis_probability_ws(0, 16, 16) == 0 and lib.pis_probability_ws(1, 0, 16) == 0
    assert lib.pis_probability_ws(1, 4097, 16) == 0 and lib.pis_probability_ws(1, 16, 4097) == 0
    assert lib.pis_probability_ws(1, 1, 1) > 0 and lib.pis_probability_ws(1, 4096, 4096) > 0
    # one partial table per block of PROB_BLOCK_PIXELS pixels: the size steps where a block is added
    n = ev.PROB_BLOCK_PIXELS
    entry = 2 * 1025 * 8  # (class, bin) entries of { uint32 count, uint32 sum of q }
    assert n % 2 == 0 and n // 2 <= 4096
    one, two = lib.pis_probability_ws(1, 2, n // 2), lib.pis_probability_ws(1, 3, n // 2)
    assert lib.pis_probability_ws(1, 1, 1) == one and 2 * entry > one >= entry     # n pixels: one block
    assert lib.pis_probability_ws(1, 3, n // 3 + 1) == two >= 2 * entry             # n + 1 pixels: two
    assert lib.pis_probability_ws(3, 2, n // 2) >= 3 * entry
    assert lib.pis_probability_ws(8, 512, 512) >= 8 * (512 * 512 // n) * entry


def _call(p=1, t=1, B=1, H=16, W=16, table=1, extra=1, ws=1, ws_bytes=None):
    """pis_probability_table with host buffers standing in for device memory: every case here must
    be refused before any launch, so nothing dereferences them."""
    lib = _hip.lib()
    n = max(B, 1) * 16 * 16
    fp = (ctypes.c_float * n)()
    ft = (ctypes.c_float * n)()
    tb = (ctypes.c_int64 * (2 * 1025 * 2 * max(B, 1)))()
    ex = (ctypes.c_int64 * (4 * max(B, 1)))()
    need = lib.pis_probability_ws(1, 16, 16)
    w = (ctypes.c_uint64 * (need // 8 + 1))()
    addr = lambda on, buf: ctypes.addressof(buf) if on else 0  # noqa: E731
    rc = lib.pis_probability_table(addr(p, fp), addr(t, ft), B, H, W, addr(table, tb), addr(extra, ex), addr(ws, w),
                                   need if ws_bytes is None else ws_bytes, 0)
    return rc, lib.pis_last_error()


@pytest.mark.parametrize("kw", [dict(p=0), dict(t=0), dict(table=0), dict(extra=0), dict(ws=0), dict(B=0),
                                dict(B=-1), dict(W=4097), dict(H=4097), dict(H=0), dict(W=0)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_argument_errors_are_reported_before_any_launch(kw):
    rc, msg = _call(**kw)
    assert rc == -1
    assert b"pis_probability_table" in msg


def test_short_workspace_is_a_workspace_error():
    rc, msg = _call(ws_bytes=16)
    assert rc == -3
    assert b"pis_probability_table" in msg and b"workspace" in msg
