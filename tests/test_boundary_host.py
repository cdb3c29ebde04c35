"""The boundary-metrics entry points (include/pis_capi.h: pis_boundary_ws, pis_boundary_metrics;
evaluate.py backends) on a GPU-less host: symbols, workspace query, argument errors before any
launch, and the host backend unchanged behind the new ``backend`` keyword."""
import ctypes

import numpy as np
import pytest
import torch

from physics_informed_image_segmentation_amd import _hip
from physics_informed_image_segmentation_amd import evaluate as ev


def test_symbols_are_bound_and_exported():
    names = _hip.exported_symbols()
    lib = _hip.lib()
    for name in ("pis_boundary_ws", "pis_boundary_metrics"):
        assert name in names
        assert hasattr(lib, name)


def test_workspace_query_runs_on_host():
    lib = _hip.lib()
    n = lib.pis_boundary_ws(8, 512, 512)
    assert n > 0
    # labels (4 B) + map (1 B) + column distance (2 B) for each pixel of the 2B images
    assert n >= 7 * 16 * 512 * 512
    assert lib.pis_boundary_ws(1, 1, 1) > 0
    assert lib.pis_boundary_ws(1, 4096, 4096) > 0
    assert lib.pis_boundary_ws(1, 4097, 16) == 0 and lib.pis_boundary_ws(0, 16, 16) == 0


def _call(p=1, t=1, B=1, H=16, W=16, tol=2, counts=1, ws=1, ws_bytes=None):
    """pis_boundary_metrics with host buffers standing in for device memory: every case here must
    be refused before any launch, so nothing dereferences them."""
    lib = _hip.lib()
    n = max(B, 1) * 16 * 16
    fp = (ctypes.c_float * n)()
    ft = (ctypes.c_float * n)()
    c = (ctypes.c_int * (6 * max(B, 1)))()
    need = lib.pis_boundary_ws(1, 16, 16)
    w = (ctypes.c_uint8 * need)()
    addr = lambda on, buf: ctypes.addressof(buf) if on else 0  # noqa: E731
    rc = lib.pis_boundary_metrics(addr(p, fp), addr(t, ft), B, H, W, 0.5, tol, addr(counts, c), 0, 0, addr(ws, w),
                                  need if ws_bytes is None else ws_bytes, 0)
    return rc, lib.pis_last_error()


@pytest.mark.parametrize("kw", [dict(p=0), dict(t=0), dict(counts=0), dict(ws=0), dict(B=0), dict(W=4097),
                                dict(H=4097), dict(H=0), dict(tol=-1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_argument_errors_are_reported_before_any_launch(kw):
    rc, msg = _call(**kw)
    assert rc == -1
    assert b"pis_boundary_metrics" in msg


def test_short_workspace_is_a_workspace_error():
    rc, msg = _call(ws_bytes=16)
    assert rc == -3
    assert b"pis_boundary_metrics" in msg


def _pair():
    t = torch.zeros(3, 1, 32, 32)
    t[0, 0, 8:20, 8:20] = 1
    t[1, 0, 4:28, 4:28] = 1
    t[1, 0, 10:20, 10:20] = 0
    p = torch.roll(t, 3, dims=-1) * 0.9 + 0.05
    return p, t


def test_device_backend_needs_cuda_tensors():
    p, t = _pair()
    with pytest.raises(ValueError):
        ev.compute_boundary_f1_batch(p, t, backend="device")
    with pytest.raises(ValueError):
        ev.compute_boundary_f1(p, t, backend="device")
    with pytest.raises(ValueError):
        ev.compute_hausdorff_distance(p, t, backend="device")
    with pytest.raises(ValueError):
        ev.compute_boundary_f1_batch(p, t, backend="gpu")


def test_host_backend_and_default_are_the_host_path():
    """On CPU tensors ``backend="host"`` and the default compute what the host functions always
    did: the values are restated here from extract_boundaries / _boundary_f1_np."""
    p, t = _pair()
    pn, tn = (p > 0.5).numpy()[:, 0], t.numpy()[:, 0]
    for tol in (0, 2, 3):
        want = np.array([ev._boundary_f1_np(ev.extract_boundaries(pn[i]), ev.extract_boundaries(tn[i]), tol, 1e-6)
                         for i in range(3)], np.float32)
        for kw in ({}, {"backend": "host"}, {"backend": "auto"}):
            got = ev.compute_boundary_f1_batch(p, t, tolerance=tol, **kw)
            assert got.dtype == torch.float32 and got.device.type == "cpu"
            np.testing.assert_array_equal(got.numpy(), want)
            assert ev.compute_boundary_f1(p, t, tolerance=tol, **kw).item() == want[0]
    assert ev.compute_hausdorff_distance(p, t) == ev.compute_hausdorff_distance(p, t, backend="host") == 3.0
    assert ev.compute_hausdorff_distance(torch.zeros(1, 1, 8, 8), t[:1, :, :8, :8], backend="host") == float("inf")


def test_train_loops_reject_a_device_scorer_on_cpu():
    import importlib
    trm = importlib.import_module("physics_informed_image_segmentation_amd.train")
    with pytest.raises(ValueError):
        trm._boundary_scorer("cpu", "device")
    sc = trm._boundary_scorer("cpu", "auto")
    try:
        assert isinstance(sc, trm._BoundaryF1Async)
    finally:
        sc.close()
